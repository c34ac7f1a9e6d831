"""Reference-free helpers for the Restormer fixtures (numpy only), used by make_golden_restormer.py (build machine, imports the
reference) and by the tests / tools (anywhere).  Like gen_common.py for the RRDB generators, the fixtures store no weights: they are
drawn from numpy's PCG64 stream in the reference's state-dict order (models/transformer/restormer.py:217-366)."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

# Restormer.__init__ defaults (restormer.py:218-230)
DEFAULTS = dict(inp_channels=3, out_channels=3, dim=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4, heads=[1, 2, 4, 8],
                ffn_expansion_factor=2.66, bias=False, LayerNorm_type="WithBias", dual_pixel_task=False)

# the fixtures: constructor arguments, batch, image size, seed
CASES = OrderedDict([
    ("a_dim8_default", dict(cfg=dict(inp_channels=3, out_channels=3, dim=8), shape=(2, 3, 32, 40), seed=101)),
    ("b_dim24_shallow", dict(cfg=dict(inp_channels=1, out_channels=1, dim=24, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1),
                             shape=(1, 1, 48, 48), seed=102)),
    ("c_bias_biasfree", dict(cfg=dict(inp_channels=2, out_channels=2, dim=8, num_blocks=[1, 2, 2, 2], num_refinement_blocks=1,
                                      bias=True, LayerNorm_type="BiasFree"), shape=(1, 2, 32, 32), seed=103)),
    ("d_ffn150", dict(cfg=dict(inp_channels=1, out_channels=1, dim=8, num_blocks=[2, 1, 1, 2], num_refinement_blocks=2,
                               heads=[2, 2, 4, 8], ffn_expansion_factor=1.5), shape=(1, 1, 24, 40), seed=104)),
])


def full_cfg(**kw) -> dict:
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    """Names and shapes of Restormer(**cfg).state_dict(), in registration order."""
    c = full_cfg(**cfg)
    d, bias, bf, f = c["dim"], c["bias"], c["LayerNorm_type"] == "BiasFree", c["ffn_expansion_factor"]
    s: "OrderedDict[str, tuple]" = OrderedDict()

    def conv(name, cout, cin, k, has_bias):
        s[name + ".weight"] = (cout, cin, k, k)
        if has_bias:
            s[name + ".bias"] = (cout,)

    def norm(name, C):
        s[name + ".body.weight"] = (C,)
        if not bf:
            s[name + ".body.bias"] = (C,)

    def blocks(prefix, n, C, heads):
        hid = int(C * f)
        for i in range(n):
            p = f"{prefix}.{i}."
            norm(p + "norm1", C)
            s[p + "attn.temperature"] = (heads, 1, 1)
            conv(p + "attn.qkv", 3 * C, C, 1, bias)
            conv(p + "attn.qkv_dwconv", 3 * C, 1, 3, bias)
            conv(p + "attn.project_out", C, C, 1, bias)
            norm(p + "norm2", C)
            conv(p + "ffn.project_in", 2 * hid, C, 1, bias)
            conv(p + "ffn.dwconv", 2 * hid, 1, 3, bias)
            conv(p + "ffn.project_out", C, hid, 1, bias)

    nb, h = c["num_blocks"], c["heads"]
    conv("patch_embed.proj", d, c["inp_channels"], 3, False)
    blocks("encoder_level1", nb[0], d, h[0])
    conv("down1_2.body.0", d // 2, d, 3, False)
    blocks("encoder_level2", nb[1], 2 * d, h[1])
    conv("down2_3.body.0", d, 2 * d, 3, False)
    blocks("encoder_level3", nb[2], 4 * d, h[2])
    conv("down3_4.body.0", 2 * d, 4 * d, 3, False)
    blocks("latent", nb[3], 8 * d, h[3])
    conv("up4_3.body.0", 16 * d, 8 * d, 3, False)
    conv("reduce_chan_level3", 4 * d, 8 * d, 1, bias)
    blocks("decoder_level3", nb[2], 4 * d, h[2])
    conv("up3_2.body.0", 8 * d, 4 * d, 3, False)
    conv("reduce_chan_level2", 2 * d, 4 * d, 1, bias)
    blocks("decoder_level2", nb[1], 2 * d, h[1])
    conv("up2_1.body.0", 4 * d, 2 * d, 3, False)
    blocks("decoder_level1", nb[0], 2 * d, h[0])
    blocks("refinement", c["num_refinement_blocks"], 2 * d, h[0])
    conv("output", c["out_channels"], 2 * d, 3, bias)
    return s


def make_state(cfg: dict, seed: int) -> "OrderedDict[str, np.ndarray]":
    """Deterministic fp32 weights in state-dict order: conv weights / biases U(-b, b), b = 1/sqrt(fan_in) (fan_in = in/groups x k x k);
    LayerNorm weights 1 + U(-0.2, 0.2), LayerNorm biases U(-0.2, 0.2), temperatures U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    fan_in = 1
    for name, shp in param_shapes(cfg).items():
        if ".body.weight" in name and len(shp) == 1:
            v = 1.0 + rng.uniform(-0.2, 0.2, size=shp)
        elif ".body.bias" in name and "norm" in name:
            v = rng.uniform(-0.2, 0.2, size=shp)
        elif name.endswith("temperature"):
            v = rng.uniform(0.5, 2.0, size=shp)
        else:
            if name.endswith(".weight"):
                fan_in = shp[1] * shp[2] * shp[3]
            b = 1.0 / np.sqrt(fan_in)
            v = rng.uniform(-b, b, size=shp)
        out[name] = v.astype(np.float32)
    return out


def make_input(shape, seed: int) -> np.ndarray:
    """a smooth field plus noise in [0, 1] (image-like: the attention's Gram is not near-degenerate)"""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = np.stack([np.stack([0.5 + 0.3 * np.sin(6.0 * xx + 3.0 * b + c) * np.cos(4.0 * yy - c) for c in range(C)]) for b in range(B)])
    return np.clip(base + 0.1 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
