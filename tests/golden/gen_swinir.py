"""Reference-free helpers for the SwinIR fixtures (numpy only), used by make_golden_swinir.py (build machine, imports the reference) and
by the tests / tools (anywhere).  Like gen_swinfir.py, the fixtures store no weights: they are drawn from numpy's PCG64 stream in the
reference's state-dict order (models/transformer/swinir.py:201-316 and the Swin blocks of modules.py); the two buffers of the state dict
(relative_position_index, attn_mask) are computed from the configuration with gen_swinfir's rel_index / shift_mask."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from gen_swinfir import make_input, rel_index, shift_mask  # noqa: F401  (make_input: re-exported for the users of this module)

# SwinIR.__init__ defaults (swinir.py:161-184; norm_layer is always nn.LayerNorm here)
DEFAULTS = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=[6, 6, 6, 6], num_heads=[6, 6, 6, 6], window_size=7,
                mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, ape=False,
                patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.0, upsampler="", resi_connection="1conv")

RGB_MEAN = (0.4488, 0.4371, 0.4040)      # swinir.py:191

# the fixtures: constructor arguments, input shape, seed
CASES = OrderedDict([
    # denoising head, pad 3 / 5, the run-time shift mask (16 x 24 != 16 x 16), the residual on the padded image, a batch of 2 in one tile
    ("a_dn_reflect", dict(cfg=dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[2, 2], num_heads=[2, 2], window_size=8,
                                   upscale=1, upsampler=""), shape=(2, 1, 13, 19), seed=301)),
    # RGB mean, 3conv in the RSTB and in conv_after_body, the shuffle-into-NCHW-with-crop store
    ("b_direct_x2_3conv_rgb", dict(cfg=dict(img_size=12, patch_size=1, in_chans=3, embed_dim=24, depths=[2], num_heads=[3], window_size=4,
                                            mlp_ratio=2.0, upscale=2, upsampler="pixelshuffledirect", resi_connection="3conv"),
                                   shape=(1, 3, 9, 10), seed=302)),
    # conv_up1 + conv_up2, no pad
    ("c_nearest_x4", dict(cfg=dict(img_size=8, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=4,
                                   upscale=4, upsampler="nearest+conv"), shape=(1, 1, 8, 12), seed=303)),
    # no conv_up2 key, pad 1 / 2, the crop after the 2x
    ("d_nearest_x2_rgb_pad", dict(cfg=dict(img_size=8, patch_size=1, in_chans=3, embed_dim=12, depths=[2], num_heads=[2], window_size=4,
                                           qkv_bias=False, upscale=2, upsampler="nearest+conv"), shape=(1, 3, 7, 10), seed=304)),
    # an odd window (49 tokens: two 32-token tiles), an odd depth, pad 6 / 1
    ("e_ps_x2_pad_w7", dict(cfg=dict(img_size=21, patch_size=1, in_chans=1, embed_dim=16, depths=[3], num_heads=[2], window_size=7,
                                     upscale=2, upsampler="pixelshuffle"), shape=(2, 1, 15, 20), seed=305)),
    # PixelShuffle(3), hidden 40, a pad on one axis only
    ("f_ps_x3_3conv", dict(cfg=dict(img_size=12, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[4], window_size=6,
                                    mlp_ratio=2.5, upscale=3, upsampler="pixelshuffle", resi_connection="3conv"),
                           shape=(1, 1, 11, 12), seed=306)),
    # effective window = min(img // patch) = 13 without shift, pad 6 / 0
    ("g_clamped_window", dict(cfg=dict(img_size=26, patch_size=2, in_chans=1, embed_dim=24, depths=[2], num_heads=[2], window_size=13,
                                       upscale=1, upsampler=""), shape=(1, 1, 20, 26), seed=307)),
    # img_range and the RGB mean on both ends of the denoising residual
    ("h_dn_imgrange255", dict(cfg=dict(img_size=8, patch_size=1, in_chans=3, embed_dim=12, depths=[2], num_heads=[2], window_size=4,
                                       upscale=1, upsampler="", img_range=255.0), shape=(1, 3, 6, 9), seed=308)),
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


def param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    """Names and shapes of SwinIR(**cfg).state_dict(), in registration order (buffers included)."""
    c = full_cfg(**cfg)
    E, cin, hid, up = c["embed_dim"], c["in_chans"], int(c["embed_dim"] * c["mlp_ratio"]), c["upscale"]
    ws, shift, res = window_of(cfg)
    s: "OrderedDict[str, tuple]" = OrderedDict()

    def lin(name, cout, cin_, k=None, bias=True):
        s[name + ".weight"] = (cout, cin_) if k is None else (cout, cin_, k, k)
        if bias:
            s[name + ".bias"] = (cout,)

    def ln(name):
        s[name + ".weight"] = (E,)
        s[name + ".bias"] = (E,)

    def resi(name):
        if c["resi_connection"] == "1conv":
            lin(name, E, E, 3)
        else:
            lin(name + ".0", E // 4, E, 3)
            lin(name + ".2", E // 4, E // 4, 1)
            lin(name + ".4", E, E // 4, 3)

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
        resi(f"layers.{i}.conv")
    ln("norm")
    resi("conv_after_body")
    if c["upsampler"] == "pixelshuffle":
        lin("conv_before_upsample.0", 64, E, 3)
        if up == 3:
            lin("upsample.0", 576, 64, 3)
        else:
            for u in range(int(np.log2(up))):
                lin(f"upsample.{2 * u}", 256, 64, 3)
        lin("conv_last", cin, 64, 3)
    elif c["upsampler"] == "pixelshuffledirect":
        lin("upsample.0", up * up * cin, E, 3)
    elif c["upsampler"] == "nearest+conv":
        lin("conv_before_upsample.0", 64, E, 3)
        lin("conv_up1", 64, 64, 3)
        if up == 4:
            lin("conv_up2", 64, 64, 3)
        lin("conv_hr", 64, 64, 3)
        lin("conv_last", cin, 64, 3)
    else:
        lin("conv_last", cin, E, 3)
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
