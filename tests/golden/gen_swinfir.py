"""Reference-free helpers for the SwinFIR fixtures (numpy only), used by make_golden_swinfir.py (build machine, imports the reference)
and by the tests / tools (anywhere).  Like gen_restormer.py, the fixtures store no weights: they are drawn from numpy's PCG64 stream
in the reference's state-dict order (models/transformer/swinfir.py:267-401 and the Swin blocks of modules.py); the two buffers of the
state dict (relative_position_index, attn_mask) are computed from the configuration."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

# SwinFIR.__init__ defaults (swinfir.py:291-313; norm_layer is always nn.LayerNorm here)
DEFAULTS = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=[6, 6, 6, 6], num_heads=[6, 6, 6, 6], window_size=7,
                mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, ape=False,
                patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.0, upsampler="", resi_connection="SFB")

# the XMM configuration: models.toml [swinfir] through the factory of model.py:187-200
XMM = dict(img_size=416, window_size=16, patch_size=32, embed_dim=180, num_heads=[6] * 6, depths=[6] * 6, upsampler="pixelshuffle",
           in_chans=1)

# the fixtures: constructor arguments, batch, image size, seed
CASES = OrderedDict([
    # the XMM shape of things: img_size // patch_size = 13 <= window_size, so the window clamps to 13 and nothing shifts
    ("a_clamped_window", dict(cfg=dict(img_size=26, patch_size=2, in_chans=1, embed_dim=24, depths=[2, 2], num_heads=[2, 2],
                                       window_size=16, upsampler="pixelshuffle"), shape=(2, 1, 26, 39), seed=201)),
    # shifted windows with the -100 mask computed for the run-time size (10 x 15 != 20 x 20), an odd W: no Nyquist bin in the C2R
    ("b_shifted_odd_w", dict(cfg=dict(img_size=20, patch_size=1, in_chans=1, embed_dim=16, depths=[2, 2], num_heads=[2, 4],
                                      window_size=5, upsampler="pixelshuffle"), shape=(1, 1, 10, 15), seed=202)),
    # three channels (the RGB mean), no qkv bias, shifted windows with the stored attn_mask (input size = img_size)
    ("c_rgb_no_qkv_bias", dict(cfg=dict(img_size=8, patch_size=1, in_chans=3, embed_dim=12, depths=[2], num_heads=[3], window_size=4,
                                        qkv_bias=False, upsampler="pixelshuffle"), shape=(2, 3, 8, 8), seed=203)),
    # resi_connection "1conv", mlp_ratio 2.5 (hidden 40), an odd block count and the PixelShuffle(3) upsampler
    ("d_1conv_mlp25_x3", dict(cfg=dict(img_size=24, patch_size=1, in_chans=1, embed_dim=16, depths=[3], num_heads=[2], window_size=6,
                                       mlp_ratio=2.5, resi_connection="1conv", upscale=3, upsampler="pixelshuffle"),
                              shape=(1, 1, 12, 18), seed=204)),
])


def full_cfg(**kw) -> dict:
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def window_of(cfg: dict):
    """(effective window, shift of the odd blocks, input_resolution) as SwinTransformerBlock.__init__ sets them (modules.py:236-239)"""
    c = full_cfg(**cfg)
    img, patch = _pair(c["img_size"]), _pair(c["patch_size"])
    res = (img[0] // patch[0], img[1] // patch[1])
    if min(res) <= c["window_size"]:
        return min(res), 0, res
    return c["window_size"], c["window_size"] // 2, res


def rel_index(ws: int) -> np.ndarray:
    yy, xx = np.meshgrid(np.arange(ws), np.arange(ws), indexing="ij")
    y, x = yy.reshape(-1), xx.reshape(-1)
    return ((y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)).astype(np.int64)


def shift_mask(h: int, w: int, ws: int, shift: int) -> np.ndarray:
    """[nW, ws^2, ws^2] float32: 0 within a region of the rolled image, -100 across regions"""
    def region(n):
        r = np.zeros(n)
        r[n - ws:n - shift] = 1
        r[n - shift:] = 2
        return r
    ids = 3 * region(h)[:, None] + region(w)[None, :]
    win = ids.reshape(h // ws, ws, w // ws, ws).transpose(0, 2, 1, 3).reshape(-1, ws * ws)
    return np.where(win[:, None, :] != win[:, :, None], -100.0, 0.0).astype(np.float32)


def param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    """Names and shapes of SwinFIR(**cfg).state_dict(), in registration order (buffers included)."""
    c = full_cfg(**cfg)
    E, cin, hid = c["embed_dim"], c["in_chans"], int(c["embed_dim"] * c["mlp_ratio"])
    ws, shift, res = window_of(cfg)
    s: "OrderedDict[str, tuple]" = OrderedDict()

    def lin(name, cout, cin_, k=None, bias=True):
        s[name + ".weight"] = (cout, cin_) if k is None else (cout, cin_, k, k)
        if bias:
            s[name + ".bias"] = (cout,)

    def ln(name):
        s[name + ".weight"] = (E,)
        s[name + ".bias"] = (E,)

    lin("conv_first", E, cin, 3)
    if c["patch_norm"]:
        ln("patch_embed.norm")
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        for j in range(depth):
            p = f"layers.{i}.residual_group.blocks.{j}."
            if j % 2 == 1 and shift > 0:
                s[p + "attn_mask"] = ((res[0] // ws) * (res[1] // ws), ws * ws, ws * ws)
            ln(p + "norm1")
            s[p + "attn.relative_position_bias_table"] = ((2 * ws - 1) ** 2, heads)
            s[p + "attn.relative_position_index"] = (ws * ws, ws * ws)
            lin(p + "attn.qkv", 3 * E, E, bias=c["qkv_bias"])
            lin(p + "attn.proj", E, E)
            ln(p + "norm2")
            lin(p + "mlp.fc1", hid, E)
            lin(p + "mlp.fc2", E, hid)
        p = f"layers.{i}.conv"
        if c["resi_connection"] == "SFB":
            lin(p + ".S.body.0", E, E, 3)
            lin(p + ".S.body.2", E, E, 3)
            lin(p + ".F.conv1.0", E // 2, E, 1)
            lin(p + ".F.fu.conv_layer", E // 2 * 2, E // 2 * 2, 1)
            lin(p + ".F.conv2", E, E // 2, 1)
            lin(p + ".fusion", E, 2 * E, 1)
        else:
            lin(p, E, E, 3)
    ln("norm")
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
    1 + U(-0.2, 0.2), LayerNorm biases U(-0.2, 0.2), bias tables U(-0.5, 0.5); the buffers as the reference computes them."""
    rng = np.random.default_rng(seed)
    ws, shift, res = window_of(cfg)
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    fan_in = 1
    for name, shp in param_shapes(cfg).items():
        if name.endswith("relative_position_index"):
            out[name] = rel_index(ws)
            continue
        if name.endswith("attn_mask"):
            out[name] = shift_mask(res[0], res[1], ws, shift)
            continue
        is_norm = "norm" in name.split(".")[-2]
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


def make_input(shape, seed: int) -> np.ndarray:
    """a smooth field plus noise in [0, 1]"""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = np.stack([np.stack([0.5 + 0.3 * np.sin(6.0 * xx + 3.0 * b + c) * np.cos(4.0 * yy - c) for c in range(C)]) for b in range(B)])
    return np.clip(base + 0.1 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
