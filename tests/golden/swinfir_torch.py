"""Plain-torch restatement of the reference SwinFIR forward (models/transformer/swinfir.py:14-441 and the Swin blocks of modules.py),
written for this project as the oracle of the engine: functional, over a state dict in the reference's key names, in whatever dtype /
device the tensors have (float64 on the CPU or the GPU for the tests, fp32 on the GPU as the eager yardstick of tools/swinfir_speed.py).
Eval-mode semantics: no dropout, no drop path.  The relative-position index and the shift mask come from the configuration, as the
reference computes them (for the run-time size)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import gen_swinfir as gs


def _lin(x, sd, name):
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def _conv(x, sd, name, padding=0):
    return F.conv2d(x, sd[name + ".weight"], sd.get(name + ".bias"), padding=padding)


def _ln(x, sd, name):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps=1e-5)


def _windows(t, ws):
    # [B, H, W, C] -> [B nW, ws^2, C], windows in row-major order
    B, H, W, C = t.shape
    return t.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _unwindows(t, ws, B, H, W):
    C = t.shape[-1]
    return t.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def window_attention(qkv, table, H, W, heads, ws, shift, scale, masked=True):
    """qkv [B, H W, 3 C] (the qkv Linear's output on the token rows, in image order), table [(2 ws - 1)^2, heads] -> [B, H W, C], the input
    of proj in image order: roll by -shift, window partition, softmax(q scale k^T + table[index] (+ the -100 shift mask)) v, window
    reverse, roll back.  masked=False leaves the shift mask out (for tests that must see it)."""
    B, L, C3 = qkv.shape
    C = C3 // 3
    hd, n = C // heads, ws * ws
    u = qkv.view(B, H, W, C3)
    if shift:
        u = torch.roll(u, shifts=(-shift, -shift), dims=(1, 2))
    qkv = _windows(u, ws).view(-1, n, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * scale, qkv[1], qkv[2]
    a = q @ k.transpose(-2, -1)
    idx = torch.from_numpy(gs.rel_index(ws)).to(qkv.device)
    a = a + table[idx.view(-1)].view(n, n, heads).permute(2, 0, 1)[None]
    if shift and masked:
        mask = torch.from_numpy(gs.shift_mask(H, W, ws, shift)).to(qkv.device, qkv.dtype)
        nw = mask.shape[0]
        a = (a.view(-1, nw, heads, n, n) + mask[None, :, None]).view(-1, heads, n, n)
    o = _unwindows((a.softmax(-1) @ v).transpose(1, 2).reshape(-1, n, C), ws, B, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B, L, C)


def _swin_block(t, sd, p, H, W, heads, ws, shift, scale):
    qkv = _lin(_ln(t, sd, p + "norm1"), sd, p + "attn.qkv")
    o = window_attention(qkv, sd[p + "attn.relative_position_bias_table"], H, W, heads, ws, shift, scale)
    t = t + _lin(o, sd, p + "attn.proj")
    return t + _lin(F.gelu(_lin(_ln(t, sd, p + "norm2"), sd, p + "mlp.fc1")), sd, p + "mlp.fc2")


def _fourier_unit(y, sd, p):
    # rfftn over (H, W), ortho; channels 2c / 2c + 1 = re / im of channel c; 1x1 conv, LeakyReLU(0.2); irfftn back to (H, W)
    B, C2, H, W = y.shape
    f = torch.fft.rfftn(y, dim=(-2, -1), norm="ortho")
    z = torch.stack((f.real, f.imag), dim=2).reshape(B, 2 * C2, H, f.shape[-1])
    z = F.leaky_relu(_conv(z, sd, p + "conv_layer"), 0.2).view(B, C2, 2, H, f.shape[-1])
    return torch.fft.irfftn(torch.complex(z[:, :, 0], z[:, :, 1]), s=(H, W), dim=(-2, -1), norm="ortho")


def _sfb(x, sd, p):
    s = _conv(F.leaky_relu(_conv(x, sd, p + "S.body.0", 1), 0.2), sd, p + "S.body.2", 1) + x
    y = F.leaky_relu(_conv(x, sd, p + "F.conv1.0"), 0.2)
    f = _conv(y + _fourier_unit(y, sd, p + "F.fu."), sd, p + "F.conv2")
    return _conv(torch.cat([s, f], 1), sd, p + "fusion")


def swinfir_forward(sd, x, **cfg):
    c = gs.full_cfg(**cfg)
    assert c["upsampler"] == "pixelshuffle" and not c["ape"]
    E = c["embed_dim"]
    ws, shift, _ = gs.window_of(cfg)
    if c["in_chans"] == 3:
        mean = torch.tensor((0.3014, 0.3152, 0.3094), dtype=torch.float32).view(1, 3, 1, 1).to(x.device, x.dtype)
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
            t = _swin_block(t, sd, f"layers.{i}.residual_group.blocks.{j}.", H, W, heads, ws, shift if j % 2 else 0, scale)
        img = t.transpose(1, 2).reshape(B, E, H, W)
        y = _sfb(img, sd, f"layers.{i}.conv.") if c["resi_connection"] == "SFB" else _conv(img, sd, f"layers.{i}.conv", 1)
        t = y.flatten(2).transpose(1, 2) + t0
    img = _ln(t, sd, "norm").transpose(1, 2).reshape(B, E, H, W)
    img = _conv(img, sd, "conv_after_body", 1) + xf
    img = F.leaky_relu(_conv(img, sd, "conv_before_upsample.0", 1), 0.01)
    r, stages = (3, 1) if c["upscale"] == 3 else (2, int(math.log2(c["upscale"])))
    for u in range(stages):
        img = F.pixel_shuffle(_conv(img, sd, f"upsample.{2 * u}", 1), r)
    return _conv(img, sd, "conv_last", 1) / c["img_range"] + mean
