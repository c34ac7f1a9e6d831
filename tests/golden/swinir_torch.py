"""Plain-torch restatement of the reference SwinIR forward (models/transformer/swinir.py:114-120, :328-395 and the Swin blocks of
modules.py), written for this project as the yardstick of the engine: functional, over a state dict in the reference's key names, in
whatever dtype / device the tensors have (float64 for the tests, fp32 on the GPU as the eager yardstick of tools/swinir_speed.py).
Eval-mode semantics.  The Swin block, the helpers and the window attention are swinfir_torch.py's."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import gen_swinir as gi
from swinfir_torch import _conv, _ln, _swin_block


def _resi(img, sd, name, three):
    if not three:
        return _conv(img, sd, name, 1)
    y = F.leaky_relu(_conv(img, sd, name + ".0", 1), 0.2)
    y = F.leaky_relu(_conv(y, sd, name + ".2"), 0.2)
    return _conv(y, sd, name + ".4", 1)


def swinir_forward(sd, x, **cfg):
    c = gi.full_cfg(**cfg)
    assert not c["ape"]
    E, up, head = c["embed_dim"], c["upscale"], c["upsampler"]
    three = c["resi_connection"] == "3conv"
    ws, shift, _ = gi.window_of(cfg)
    H0, W0 = x.shape[2:]
    w = c["window_size"]
    x = F.pad(x, (0, (w - W0 % w) % w, 0, (w - H0 % w) % w), "reflect")
    if c["in_chans"] == 3:
        mean = torch.tensor(gi.RGB_MEAN, dtype=torch.float32).view(1, 3, 1, 1).to(x.device, x.dtype)
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
        t = _resi(img, sd, f"layers.{i}.conv", three).flatten(2).transpose(1, 2) + t0
    img = _ln(t, sd, "norm").transpose(1, 2).reshape(B, E, H, W)
    img = _resi(img, sd, "conv_after_body", three) + xf
    if head == "pixelshuffle":
        img = F.leaky_relu(_conv(img, sd, "conv_before_upsample.0", 1), 0.01)
        r, stages = (3, 1) if up == 3 else (2, int(math.log2(up)))
        for u in range(stages):
            img = F.pixel_shuffle(_conv(img, sd, f"upsample.{2 * u}", 1), r)
        y = _conv(img, sd, "conv_last", 1)
    elif head == "pixelshuffledirect":
        y = F.pixel_shuffle(_conv(img, sd, "upsample.0", 1), up)
    elif head == "nearest+conv":
        img = F.leaky_relu(_conv(img, sd, "conv_before_upsample.0", 1), 0.01)
        img = F.leaky_relu(_conv(F.interpolate(img, scale_factor=2, mode="nearest"), sd, "conv_up1", 1), 0.2)
        if up == 4:
            img = F.leaky_relu(_conv(F.interpolate(img, scale_factor=2, mode="nearest"), sd, "conv_up2", 1), 0.2)
        y = _conv(F.leaky_relu(_conv(img, sd, "conv_hr", 1), 0.2), sd, "conv_last", 1)
    else:
        y = x + _conv(img, sd, "conv_last", 1)
    y = y / c["img_range"] + mean
    return y[:, :, :H0 * up, :W0 * up]
