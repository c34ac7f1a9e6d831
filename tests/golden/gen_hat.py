"""Reference-free helpers for the HAT fixtures (numpy only), used by make_golden_hat.py (build machine, imports the reference) and by
the tests / tools (anywhere).  Like gen_swinfir.py, the fixtures store no weights: they are drawn from numpy's PCG64 stream in the
reference's state-dict order (models/transformer/hat.py:694-785 and its HAB / OCAB / CAB blocks); the two buffers of the state dict
(relative_position_index_SA, relative_position_index_OCA) are computed from the configuration."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from gen_swinfir import make_input, rel_index, shift_mask  # noqa: F401  (the same inputs, SA index and run-time shift mask)

# HAT.__init__ defaults (hat.py:642-669; norm_layer is always nn.LayerNorm here)
DEFAULTS = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=[6, 6, 6, 6], num_heads=[6, 6, 6, 6], window_size=7,
                compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, ape=False, patch_norm=True, use_checkpoint=False, upscale=2,
                img_range=1.0, upsampler="", resi_connection="1conv")

# the XMM configuration: models.toml [hat] through the factory of model.py:216-229
XMM = dict(img_size=416, window_size=16, patch_size=16, embed_dim=180, num_heads=[6] * 6, depths=[6] * 6, upsampler="pixelshuffle",
           in_chans=1)

_PS = dict(patch_size=1, upsampler="pixelshuffle")

# the fixtures: constructor arguments, batch, image size, seed
CASES = OrderedDict([
    # shifted windows (mask of the run-time size 16 x 24 != 16 x 16) and the OCAB with 12 x 12 keys per 8 x 8 window, head dim 30
    ("a_shifted_ocab", dict(cfg=dict(_PS, img_size=16, in_chans=1, embed_dim=60, depths=[2, 2], num_heads=[2, 2], window_size=8),
                            shape=(2, 1, 16, 24), seed=301)),
    # odd window 5 with 7 x 7 keys, an odd width, the "identity" branches
    ("b_odd_sizes", dict(cfg=dict(_PS, img_size=32, in_chans=1, embed_dim=32, depths=[2], num_heads=[2], window_size=5, overlap_ratio=0.4,
                                  squeeze_factor=8, resi_connection="identity"), shape=(1, 1, 10, 15), seed=302)),
    # three channels (the RGB mean), no qkv bias, mlp_ratio 2.5, an odd block count, two PixelShuffle(2) stages
    ("c_rgb", dict(cfg=dict(_PS, img_size=16, in_chans=3, embed_dim=36, depths=[3], num_heads=[3], window_size=4, qkv_bias=False,
                            mlp_ratio=2.5, compress_ratio=2, squeeze_factor=8, upscale=4), shape=(2, 3, 8, 12), seed=303)),
    # img_size // patch_size == window_size: no block shifts
    ("d_no_shift", dict(cfg=dict(_PS, img_size=8, in_chans=1, embed_dim=32, depths=[2], num_heads=[2], window_size=8, squeeze_factor=8),
                        shape=(1, 1, 8, 8), seed=304)),
    # a given qk_scale, conv_scale 0.5 (the CAB branch at full weight in the error budget), img_range 255
    ("e_scales", dict(cfg=dict(_PS, img_size=16, in_chans=1, embed_dim=32, depths=[2], num_heads=[2], window_size=4, squeeze_factor=8,
                               qk_scale=0.3, conv_scale=0.5, img_range=255.0), shape=(1, 1, 12, 16), seed=305)),
    ("e_scales_x3", dict(cfg=dict(_PS, img_size=16, in_chans=1, embed_dim=32, depths=[2], num_heads=[2], window_size=4, squeeze_factor=8,
                                  qk_scale=0.3, conv_scale=0.5, img_range=255.0, upscale=3), shape=(1, 1, 12, 16), seed=306)),
    # the XMM block shape: embed 180, 6 heads of 30, 16 x 16 windows against 24 x 24 keys
    ("f_xmm_block", dict(cfg=dict(_PS, img_size=32, in_chans=1, embed_dim=180, depths=[2], num_heads=[6], window_size=16),
                         shape=(1, 1, 32, 48), seed=307)),
])


def full_cfg(**kw) -> dict:
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def window_of(cfg: dict):
    """(window, shift of the odd blocks, overlap window): the shift is decided at construction from img_size // patch_size
    (HAB.__init__, hat.py:186-189); a resolution below the window is not a valid configuration"""
    c = full_cfg(**cfg)
    img, patch = _pair(c["img_size"]), _pair(c["patch_size"])
    res = min(img[0] // patch[0], img[1] // patch[1])
    ws = c["window_size"]
    assert res >= ws
    return ws, (0 if res <= ws else ws // 2), ws + int(ws * c["overlap_ratio"])


def rel_index_oca(ws: int, ow: int) -> np.ndarray:
    """[ws^2, ow^2]: (dy + ws - ow + 1) (ws + ow - 1) + (dx + ws - ow + 1), (dy, dx) = key position in the overlapping window minus
    query position in the window; entries can be negative (they index the table from its end), hat.py:805-834"""
    qy, qx = [a.reshape(-1) for a in np.meshgrid(np.arange(ws), np.arange(ws), indexing="ij")]
    ky, kx = [a.reshape(-1) for a in np.meshgrid(np.arange(ow), np.arange(ow), indexing="ij")]
    s = ws - ow + 1
    return ((ky[None, :] - qy[:, None] + s) * (ws + ow - 1) + (kx[None, :] - qx[:, None] + s)).astype(np.int64)


def param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    """Names and shapes of HAT(**cfg).state_dict(), in registration order (buffers included)."""
    c = full_cfg(**cfg)
    E, cin, hid = c["embed_dim"], c["in_chans"], int(c["embed_dim"] * c["mlp_ratio"])
    Cc, Cs = E // c["compress_ratio"], E // c["squeeze_factor"]
    ws, _, ow = window_of(cfg)
    s: "OrderedDict[str, tuple]" = OrderedDict()

    def lin(name, cout, cin_, k=None, bias=True):
        s[name + ".weight"] = (cout, cin_) if k is None else (cout, cin_, k, k)
        if bias:
            s[name + ".bias"] = (cout,)

    def ln(name):
        s[name + ".weight"] = (E,)
        s[name + ".bias"] = (E,)

    s["relative_position_index_SA"] = (ws * ws, ws * ws)
    s["relative_position_index_OCA"] = (ws * ws, ow * ow)
    lin("conv_first", E, cin, 3)
    if c["patch_norm"]:
        ln("patch_embed.norm")
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        for j in range(depth):
            p = f"layers.{i}.residual_group.blocks.{j}."
            ln(p + "norm1")
            s[p + "attn.relative_position_bias_table"] = ((2 * ws - 1) ** 2, heads)
            lin(p + "attn.qkv", 3 * E, E, bias=c["qkv_bias"])
            lin(p + "attn.proj", E, E)
            lin(p + "conv_block.cab.0", Cc, E, 3)
            lin(p + "conv_block.cab.2", E, Cc, 3)
            lin(p + "conv_block.cab.3.attention.1", Cs, E, 1)
            lin(p + "conv_block.cab.3.attention.3", E, Cs, 1)
            ln(p + "norm2")
            lin(p + "mlp.fc1", hid, E)
            lin(p + "mlp.fc2", E, hid)
        p = f"layers.{i}.residual_group.overlap_attn."
        s[p + "relative_position_bias_table"] = ((ws + ow - 1) ** 2, heads)
        ln(p + "norm1")
        lin(p + "qkv", 3 * E, E, bias=c["qkv_bias"])
        lin(p + "proj", E, E)
        ln(p + "norm2")
        lin(p + "mlp.fc1", hid, E)
        lin(p + "mlp.fc2", E, hid)
        if c["resi_connection"] == "1conv":
            lin(f"layers.{i}.conv", E, E, 3)
    ln("norm")
    if c["resi_connection"] == "1conv":
        lin("conv_after_body", E, E, 3)
    lin("conv_before_upsample.0", 64, E, 3)
    if c["upscale"] == 3:
        lin("upsample.0", 576, 64, 3)
    else:
        for u in range(int(np.log2(c["upscale"]))):
            lin(f"upsample.{2 * u}", 256, 64, 3)
    lin("conv_last", cin, 64, 3)
    return s


def make_state(cfg: dict, seed: int) -> "OrderedDict[str, np.ndarray]":
    """Deterministic weights in state-dict order: Linear / conv weights and biases U(-b, b), b = 1/sqrt(fan_in); LayerNorm weights
    1 + U(-0.2, 0.2), LayerNorm biases U(-0.2, 0.2), bias tables U(-0.5, 0.5) so that a wrong index shows; the buffers as the reference
    computes them."""
    rng = np.random.default_rng(seed)
    ws, _, ow = window_of(cfg)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    fan_in = 1
    for name, shp in param_shapes(cfg).items():
        if name == "relative_position_index_SA":
            out[name] = rel_index(ws)
            continue
        if name == "relative_position_index_OCA":
            out[name] = rel_index_oca(ws, ow)
            continue
        is_norm = name.endswith("relative_position_bias_table") is False and "norm" in name.split(".")[-2]
        if is_norm and name.endswith(".weight"):
            v = 1.0 + rng.uniform(-0.2, 0.2, size=shp)
        elif is_norm:
            v = rng.uniform(-0.2, 0.2, size=shp)
        elif name.endswith("relative_position_bias_table"):
            v = rng.uniform(-0.5, 0.5, size=shp)
        else:
            if name.endswith(".weight"):
                fan_in = int(np.prod(shp[1:]))
            b = 1.0 / np.sqrt(fan_in)
            v = rng.uniform(-b, b, size=shp)
        out[name] = v.astype(np.float32)
    return out
