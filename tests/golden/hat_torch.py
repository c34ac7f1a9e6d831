"""Plain-torch restatement of the reference HAT forward (models/transformer/hat.py:10-913), written for this project as the oracle of the
engine: functional, over a state dict in the reference's key names, in whatever dtype / device the tensors have (float64 on the CPU or the
GPU for the tests, fp32 on the GPU as the eager yardstick of tools/hat_speed.py).  Eval-mode semantics: no dropout, no drop path.  The two
relative-position indices and the shift mask come from the configuration, the mask for the run-time size, as the reference computes them.

The overlapping cross-attention is restated by gathering: the key / value window of window (wy, wx) is the (ow x ow) patch of the
zero-padded k / v maps at (wy ws, wx ws), which is what the reference's nn.Unfold(kernel ow, stride ws, padding (ow - ws) / 2) yields."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import gen_hat as gh
from swinfir_torch import _conv, _lin, _ln, _unwindows, _windows, window_attention


def _mlp(t, sd, p):
    return t + _lin(F.gelu(_lin(_ln(t, sd, p + "norm2"), sd, p + "mlp.fc1")), sd, p + "mlp.fc2")


def channel_attention(x, sd, p):
    """x [B, C, H, W] -> x * sigmoid(conv1x1(relu(conv1x1(mean over H, W))))"""
    y = x.mean((2, 3), keepdim=True)
    y = torch.sigmoid(_conv(F.relu(_conv(y, sd, p + "attention.1")), sd, p + "attention.3"))
    return x * y


def cab(u, sd, p):
    """u [B, C, H, W]: conv3x3 -> GELU -> conv3x3 -> channel attention"""
    y = _conv(F.gelu(_conv(u, sd, p + "cab.0", 1)), sd, p + "cab.2", 1)
    return channel_attention(y, sd, p + "cab.3.")


def _hab(t, sd, p, H, W, heads, ws, shift, scale, conv_scale):
    B, L, C = t.shape
    u = _ln(t, sd, p + "norm1")
    conv_x = cab(u.view(B, H, W, C).permute(0, 3, 1, 2), sd, p + "conv_block.").permute(0, 2, 3, 1).reshape(B, L, C)
    o = window_attention(_lin(u, sd, p + "attn.qkv"), sd[p + "attn.relative_position_bias_table"], H, W, heads, ws, shift, scale)
    t = t + _lin(o, sd, p + "attn.proj") + conv_x * conv_scale
    return _mlp(t, sd, p)


def ocab_attention(qkv, table, H, W, heads, ws, ow, scale):
    """qkv [B, H W, 3 C] (the qkv Linear's output on the token rows), table [(ws + ow - 1)^2, heads] -> [B, H W, C], the input of proj"""
    B, L, C3 = qkv.shape
    C = C3 // 3
    hd, nq, nk, pad = C // heads, ws * ws, ow * ow, (ow - ws) // 2
    q, k, v = qkv.view(B, H, W, 3, C).unbind(3)
    nwy, nwx = H // ws, W // ws

    def overlapping(m):
        mp = F.pad(m, (0, 0, pad, pad, pad, pad))                         # zeros around the image
        w = mp.unfold(1, ow, ws).unfold(2, ow, ws)                       # [B, nwy, nwx, C, ow, ow]
        return w.permute(0, 1, 2, 4, 5, 3).reshape(B * nwy * nwx, nk, heads, hd).transpose(1, 2)

    qw = _windows(q, ws).view(-1, nq, heads, hd).transpose(1, 2) * scale
    a = qw @ overlapping(k).transpose(-2, -1)
    idx = torch.from_numpy(gh.rel_index_oca(ws, ow)).to(qkv.device)
    a = a + table[idx.view(-1)].view(nq, nk, heads).permute(2, 0, 1)[None]
    o = (a.softmax(-1) @ overlapping(v)).transpose(1, 2).reshape(-1, nq, C)
    return _unwindows(o, ws, B, H, W).reshape(B, L, C)


def _ocab(t, sd, p, H, W, heads, ws, ow, scale):
    qkv = _lin(_ln(t, sd, p + "norm1"), sd, p + "qkv")
    o = ocab_attention(qkv, sd[p + "relative_position_bias_table"], H, W, heads, ws, ow, scale)
    t = _lin(o, sd, p + "proj") + t
    return _mlp(t, sd, p)


def hat_forward(sd, x, **cfg):
    c = gh.full_cfg(**cfg)
    assert c["upsampler"] == "pixelshuffle" and not c["ape"]
    E = c["embed_dim"]
    ws, shift, ow = gh.window_of(cfg)
    if c["in_chans"] == 3:
        mean = torch.tensor((0.4488, 0.4371, 0.4040), dtype=torch.float32).view(1, 3, 1, 1).to(x.device, x.dtype)
    else:
        mean = torch.zeros(1, 1, 1, 1, dtype=x.dtype, device=x.device)
    x = (x - mean) * c["img_range"]
    xf = _conv(x, sd, "conv_first", 1)
    B, _, H, W = xf.shape
    t = xf.flatten(2).transpose(1, 2)
    if c["patch_norm"]:
        t = _ln(t, sd, "patch_embed.norm")
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        scale = c["qk_scale"] or (E // heads) ** -0.5
        t0 = t
        for j in range(depth):
            t = _hab(t, sd, f"layers.{i}.residual_group.blocks.{j}.", H, W, heads, ws, shift if j % 2 else 0, scale, c["conv_scale"])
        t = _ocab(t, sd, f"layers.{i}.residual_group.overlap_attn.", H, W, heads, ws, ow, scale)
        if c["resi_connection"] == "1conv":
            t = _conv(t.transpose(1, 2).reshape(B, E, H, W), sd, f"layers.{i}.conv", 1).flatten(2).transpose(1, 2)
        t = t + t0
    img = _ln(t, sd, "norm").transpose(1, 2).reshape(B, E, H, W)
    if c["resi_connection"] == "1conv":
        img = _conv(img, sd, "conv_after_body", 1)
    img = img + xf
    img = F.leaky_relu(_conv(img, sd, "conv_before_upsample.0", 1), 0.01)
    r, stages = (3, 1) if c["upscale"] == 3 else (2, int(math.log2(c["upscale"])))
    for u in range(stages):
        img = F.pixel_shuffle(_conv(img, sd, f"upsample.{2 * u}", 1), r)
    return _conv(img, sd, "conv_last", 1) / c["img_range"] + mean
