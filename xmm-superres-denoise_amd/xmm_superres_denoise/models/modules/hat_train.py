"""TrainableHAT: the reference's HAT forward (models/transformer/hat.py:867-913 with its RHAG / HAB / CAB / OCAB blocks) for upsampler
"pixelshuffle" and resi_connection "1conv" or "identity", composed in Python from the differentiable ops of xmm_superres_denoise/ops.py
(hand-written HIP forward and backward: linear, conv3x3, layer_norm, window_attention and HAT's own overlap_attention and
channel_attention), with torch's autograd holding the graph.  Plain torch ops do the plumbing only: the mean / img_range affine,
residual adds, the conv_scale product, reshapes / transposes, pixel_shuffle, DropPath's per-sample scale, the optional clamp.

It WRAPS a models.HAT and shares its Parameter objects exactly as TrainableSwinFIR wraps a models.SwinFIR: state-dict key names, order,
init and checkpoints are the reference's (the wrapper's state_dict / load_state_dict are the wrapped module's), and after training the
wrapped module's fused forward (csrc/hat.hip) re-packs and sees the new weights.  models.HAT itself stays forward-only and keeps its
refusal.

Refused in the constructor, by name: anything that is not a models.HAT, and dropout rates other than 0.  models.HAT pads nothing, so
sizes off the window grid are refused in the wrapped module's own words.

DropPath, `generator`, `last_drop_masks`, `clamp` and the pixel-shuffle tail are TrainableSwinIR's, in one copy (swinir_train.py:
TrainableSwin).  As in the reference, a HAB drops its attention branch and its MLP branch (two masks per HAB in `last_drop_masks`),
never its CAB branch conv_x, and an OCAB drops nothing: a sample whose attention branch was dropped still sends a gradient to the
block's conv_block.
"""
from __future__ import annotations

import torch

from xmm_superres_denoise import ops
from xmm_superres_denoise.engine import XsdError

from .hat import HAT
from .swinir_train import TrainableSwin


class TrainableHAT(TrainableSwin):
    def __init__(self, module: HAT, drop_path_rate: float | None = None, generator: torch.Generator | None = None,
                 clamp: bool = False):
        """`drop_path_rate`: None takes the wrapped module's constructor argument.  `clamp`: clamp the output to [0, 1] as Model.forward
        does (models/model.py:48-49)."""
        super().__init__()
        if not isinstance(module, HAT):
            raise TypeError(f"TrainableHAT wraps a models.HAT (got {type(module).__name__})")
        self._wrap(module, drop_path_rate, generator, clamp)

    def _mlp(self, t: torch.Tensor, blk, p: float | None) -> torch.Tensor:
        h = ops.linear(ops.layer_norm(t, blk.norm2.weight, blk.norm2.bias), blk.mlp.fc1.weight, blk.mlp.fc1.bias, act="gelu")
        h = ops.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
        return t + (h if p is None else self._drop(h, p))

    def _features(self, x: torch.Tensor, window: int | None = None) -> torch.Tensor:
        """forward_features (hat.py:867-898) with conv_first and the long skip around it: the scaled image x [B, C, H, W] -> [B, H, W, E]
        token-major.  Per RHAG: the HABs, the OCAB, then the group's conv ("1conv") or nothing ("identity"), plus the group's input."""
        m = self.module
        E = m.embed_dim
        B, _, H, W = x.shape
        conv1 = m.resi_connection == "1conv"
        ow = m.window + int(m.window * m.overlap_ratio)
        xf = ops.conv3x3(x.permute(0, 2, 3, 1).contiguous(), m.conv_first.weight, m.conv_first.bias)       # [B, H, W, E] token-major
        t = xf.view(B, H * W, E)
        if m.patch_norm:
            t = ops.layer_norm(t, m.patch_embed.norm.weight, m.patch_embed.norm.bias)
        k = 0
        for i, layer in enumerate(m.layers):
            heads = m.num_heads[i]
            scale = m.qk_scale or (E // heads) ** -0.5
            t0 = t
            for blk in layer.residual_group.blocks:                                                        # HAB (hat.py:220-271)
                a, cab = blk.attn, blk.conv_block.cab
                u = ops.layer_norm(t, blk.norm1.weight, blk.norm1.bias)
                c = ops.conv3x3(u.view(B, H, W, E), cab[0].weight, cab[0].bias, act="gelu")
                c = ops.conv3x3(c, cab[2].weight, cab[2].bias).view(B, H * W, E)
                sq = cab[3].attention
                conv_x = ops.channel_attention(c, sq[1].weight, sq[1].bias, sq[3].weight, sq[3].bias)
                qkv = ops.linear(u, a.qkv.weight, a.qkv.bias)
                o = ops.window_attention(qkv, a.relative_position_bias_table, H, W, heads, blk.window_size, blk.shift_size, scale)
                t = t + self._drop(ops.linear(o, a.proj.weight, a.proj.bias), self.drop_path[k]) + conv_x * blk.conv_scale
                t = self._mlp(t, blk, self.drop_path[k])
                k += 1
            oc = layer.residual_group.overlap_attn                                                         # OCAB (hat.py:326-396)
            qkv = ops.linear(ops.layer_norm(t, oc.norm1.weight, oc.norm1.bias), oc.qkv.weight, oc.qkv.bias)
            o = ops.overlap_attention(qkv, oc.relative_position_bias_table, H, W, heads, m.window, ow, scale)
            t = self._mlp(ops.linear(o, oc.proj.weight, oc.proj.bias) + t, oc, None)
            if conv1:
                t = ops.conv3x3(t.view(B, H, W, E), layer.conv.weight, layer.conv.bias).view(B, H * W, E)
            t = t + t0
        t = ops.layer_norm(t, m.norm.weight, m.norm.bias).view(B, H, W, E)
        if conv1:
            t = ops.conv3x3(t, m.conv_after_body.weight, m.conv_after_body.bias)
        return t + xf

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        m = self.module
        self._check_input(x)
        H, W = int(x.shape[2]), int(x.shape[3])
        # the sizes models.HAT.forward refuses, in its words
        if H % m.window or W % m.window:
            raise XsdError(f"HAT needs H and W that are multiples of the window size {m.window} (window_partition; the reference does "
                           f"not pad); got {H} x {W}")
        self.last_drop_masks = []
        mean = self._mean_like(x)
        y = self._pixelshuffle_tail(self._features((x - mean) * m.img_range))
        y = (y / m.img_range + mean).contiguous()
        return y.clamp(0.0, 1.0) if self.clamp else y
