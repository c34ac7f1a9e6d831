"""Plain-torch restatement of the reference Restormer forward (models/transformer/restormer.py:25-406), written for this project as
the oracle of the engine: functional, over a state dict in the reference's key names, in whatever dtype / device the tensors have
(float64 on the CPU or the GPU for the tests, fp32 on the GPU as the eager yardstick of tools/restormer_speed.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _layer_norm(x, sd, name, bias_free):
    # over the channel dim of each pixel: biased variance, eps 1e-5 inside the square root (:36-58)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    w = sd[name + ".body.weight"].view(1, -1, 1, 1)
    if bias_free:
        return x / torch.sqrt(var + 1e-5) * w
    return (x - mu) / torch.sqrt(var + 1e-5) * w + sd[name + ".body.bias"].view(1, -1, 1, 1)


def _conv(x, sd, name, padding=0, groups=1):
    return F.conv2d(x, sd[name + ".weight"], sd.get(name + ".bias"), padding=padding, groups=groups)


def channel_attention(qkv, temperature, heads):
    """qkv [B, 3 C, H, W] as the depthwise conv leaves it, temperature [heads, 1, 1] -> softmax(normalize(q) normalize(k)^T temperature) v,
    [B, C, H, W], the input of project_out (:126-139)"""
    B, C3, H, W = qkv.shape
    C = C3 // 3
    q, k, v = (t.reshape(B, heads, C // heads, H * W) for t in qkv.chunk(3, dim=1))
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)          # F.normalize(dim=-1), eps 1e-12
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    attn = (q @ k.transpose(-2, -1)) * temperature
    return (attn.softmax(dim=-1) @ v).reshape(B, C, H, W)


def _attention(x, sd, p, heads):
    C = x.shape[1]
    qkv = _conv(_conv(x, sd, p + "qkv"), sd, p + "qkv_dwconv", padding=1, groups=3 * C)
    return _conv(channel_attention(qkv, sd[p + "temperature"], heads), sd, p + "project_out")


def _ffn(x, sd, p):
    h = _conv(x, sd, p + "project_in")
    x1, x2 = _conv(h, sd, p + "dwconv", padding=1, groups=h.shape[1]).chunk(2, dim=1)
    return _conv(F.gelu(x1) * x2, sd, p + "project_out")


def _blocks(x, sd, prefix, n, heads, bias_free):
    for i in range(n):
        p = f"{prefix}.{i}."
        x = x + _attention(_layer_norm(x, sd, p + "norm1", bias_free), sd, p + "attn.", heads)
        x = x + _ffn(_layer_norm(x, sd, p + "norm2", bias_free), sd, p + "ffn.")
    return x


def restormer_forward(sd: dict, x: torch.Tensor, num_blocks=(4, 6, 6, 8), num_refinement_blocks=4, heads=(1, 2, 4, 8),
                      LayerNorm_type="WithBias", **_unused) -> torch.Tensor:
    """Restormer.forward (:368-406) without dual_pixel_task; sd: name -> tensor (same dtype / device as x)."""
    bf = LayerNorm_type == "BiasFree"
    nb, h = list(num_blocks), list(heads)
    e1 = _blocks(_conv(x, sd, "patch_embed.proj", padding=1), sd, "encoder_level1", nb[0], h[0], bf)
    e2 = _blocks(F.pixel_unshuffle(_conv(e1, sd, "down1_2.body.0", padding=1), 2), sd, "encoder_level2", nb[1], h[1], bf)
    e3 = _blocks(F.pixel_unshuffle(_conv(e2, sd, "down2_3.body.0", padding=1), 2), sd, "encoder_level3", nb[2], h[2], bf)
    lat = _blocks(F.pixel_unshuffle(_conv(e3, sd, "down3_4.body.0", padding=1), 2), sd, "latent", nb[3], h[3], bf)
    d3 = torch.cat([F.pixel_shuffle(_conv(lat, sd, "up4_3.body.0", padding=1), 2), e3], 1)
    d3 = _blocks(_conv(d3, sd, "reduce_chan_level3"), sd, "decoder_level3", nb[2], h[2], bf)
    d2 = torch.cat([F.pixel_shuffle(_conv(d3, sd, "up3_2.body.0", padding=1), 2), e2], 1)
    d2 = _blocks(_conv(d2, sd, "reduce_chan_level2"), sd, "decoder_level2", nb[1], h[1], bf)
    d1 = torch.cat([F.pixel_shuffle(_conv(d2, sd, "up2_1.body.0", padding=1), 2), e1], 1)
    d1 = _blocks(d1, sd, "decoder_level1", nb[0], h[0], bf)
    d1 = _blocks(d1, sd, "refinement", num_refinement_blocks, h[0], bf)
    return _conv(d1, sd, "output", padding=1) + x
