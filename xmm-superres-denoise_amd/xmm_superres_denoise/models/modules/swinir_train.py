"""TrainableSwinIR: the reference's SwinIR forward (models/transformer/swinir.py:350-395 with the Swin blocks of modules.py) composed in
Python from the differentiable ops of xmm_superres_denoise/ops.py (hand-written HIP forward and backward: linear, conv3x3, layer_norm,
window_attention), with torch's autograd holding the graph.  Plain torch ops do the plumbing only: reflect pad, crop, the mean /
img_range affine, residual adds, reshapes / transposes, pixel_shuffle, DropPath's per-sample scale, the optional clamp.

It WRAPS a models.SwinIR and shares its Parameter objects: state-dict key names, order, init and checkpoints are the reference's (the
wrapper's state_dict / load_state_dict are the wrapped module's), and after training the wrapped module's fused forward
(csrc/swinir.hip) re-packs and sees the new weights.  models.SwinIR itself stays forward-only and keeps its refusal.

Supported: upsampler "" (denoising) and "pixelshuffle" (every upscale the module takes), resi_connection "1conv", patch_norm on or off,
qkv_bias on or off, any in_chans.  Refused in the constructor, by name: "pixelshuffledirect", "nearest+conv", "3conv", dropout rates
other than 0.

DropPath (modules.py drop_path): in train() mode with drop_path_rate > 0 each residual branch of block k is dropped per sample with
probability linspace(0, rate, sum(depths))[k] and the kept ones scaled by 1 / keep; the masks are drawn from `generator` (or torch's
default one) and those of the last forward are kept in `last_drop_masks` (two per block: attention branch, MLP branch; all-ones where the
rate is 0).  In eval() it is the identity.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from xmm_superres_denoise import ops
from xmm_superres_denoise.engine import XsdError

from .flat_params import inference_refusal, tracks_version
from .swinir import SwinIR


def drop_path_schedule(depths, rate: float) -> list:
    """[x.item() for x in torch.linspace(0, rate, sum(depths))] (swinir.py:226): the drop probability of every block, in order"""
    return [float(v) for v in torch.linspace(0, float(rate), int(sum(depths)))]


class TrainableSwin(nn.Module):
    """What TrainableSwinIR and TrainableSwinFIR (swinfir_train.py) share: the wrapped module's names, DropPath, the input checks, the
    RSTB loop with "1conv" and the pixel-shuffle tail.  A subclass checks what it wraps, then calls _wrap."""

    def _wrap(self, module, drop_path_rate, generator, clamp):
        name = type(self).__name__
        for n in ("drop_rate", "attn_drop_rate"):
            if float(getattr(module, n, 0.0)) != 0.0:
                raise NotImplementedError(f"{name}: {n} = {getattr(module, n)} is not supported (dropout rates other than 0 are not "
                                          "on the MI355X engine; DropPath is: drop_path_rate)")
        rate = float(getattr(module, "drop_path_rate", 0.0) if drop_path_rate is None else drop_path_rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"{name}: drop_path_rate {rate} is outside [0, 1)")
        self.module = module
        self.drop_path_rate = rate
        self.drop_path = drop_path_schedule(module.depths, rate)
        self.generator = generator
        self.clamp = bool(clamp)
        self.last_drop_masks = []
        self._mean_dev = None

    # ---- the wrapped module's names --------------------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        return self.module.state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        return self.module.load_state_dict(*args, **kwargs)

    def __getstate__(self):
        """copies and pickles carry the wrapped module (by its own rule) and the configuration, not the generator or the last masks"""
        st = self.__dict__.copy()
        st["generator"] = None
        st["last_drop_masks"] = []
        st["_mean_dev"] = None
        return st

    def _mean_like(self, x: torch.Tensor) -> torch.Tensor:
        """the wrapped module's per-channel mean (a host tensor, as in the reference) on x's device: uploaded once and kept.  An upload
        per forward is a copy from pageable host memory, which holds the host until x's stream has drained: every training step would
        wait for the device instead of running ahead of it."""
        kept = getattr(self, "_mean_dev", None)
        if kept is None or kept.device != x.device or kept.dtype != x.dtype:
            kept = self._mean_dev = self.module.mean.to(device=x.device, dtype=x.dtype)
        return kept

    # ---- forward ---------------------------------------------------------------------------------------------------
    def _drop(self, t: torch.Tensor, p: float) -> torch.Tensor:
        B = t.shape[0]
        if not self.training or self.drop_path_rate == 0.0:
            return t
        if p == 0.0:
            self.last_drop_masks.append(torch.ones(B, device=t.device))
            return t
        g = self.generator
        keep = 1.0 - p
        r = torch.rand(B, generator=g, device=g.device if g is not None else t.device).to(t.device)
        mask = torch.floor(keep + r)                      # random_tensor.floor_() of drop_path
        self.last_drop_masks.append(mask)
        return t / keep * mask.view(B, 1, 1)

    def _check_input(self, x: torch.Tensor):
        self.module._check_input(x, self.module.in_chans)
        if not x.is_cuda:
            raise XsdError("the MI355X engine needs CUDA(HIP) tensors; there is no CPU fallback")
        if torch.is_grad_enabled() and not all(tracks_version(p) for p in self.module.parameters()):
            raise inference_refusal(type(self).__name__, f"the wrapped {type(self.module).__name__}'s")

    def _features(self, x: torch.Tensor, window: int | None = None) -> torch.Tensor:
        """conv_first .. conv_after_body + conv_first's output on the scaled image x [B, C, H, W] -> [B, H, W, E] token-major.  `window`:
        the window of every block, or None for each block's own `window_size`."""
        m = self.module
        E = m.embed_dim
        B, _, H, W = x.shape
        xf = ops.conv3x3(x.permute(0, 2, 3, 1).contiguous(), m.conv_first.weight, m.conv_first.bias)       # [B, H, W, E] token-major
        t = xf.view(B, H * W, E)
        if m.patch_norm:
            t = ops.layer_norm(t, m.patch_embed.norm.weight, m.patch_embed.norm.bias)
        k = 0
        for i, layer in enumerate(m.layers):
            heads = m.num_heads[i]
            scale = m.qk_scale or (E // heads) ** -0.5
            t0 = t
            for blk in layer.residual_group.blocks:
                a = blk.attn
                ws = blk.window_size if window is None else window
                qkv = ops.linear(ops.layer_norm(t, blk.norm1.weight, blk.norm1.bias), a.qkv.weight, a.qkv.bias)
                o = ops.window_attention(qkv, a.relative_position_bias_table, H, W, heads, ws, blk.shift_size, scale)
                t = t + self._drop(ops.linear(o, a.proj.weight, a.proj.bias), self.drop_path[k])
                h = ops.linear(ops.layer_norm(t, blk.norm2.weight, blk.norm2.bias), blk.mlp.fc1.weight, blk.mlp.fc1.bias, act="gelu")
                t = t + self._drop(ops.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias), self.drop_path[k])
                k += 1
            t = ops.conv3x3(t.view(B, H, W, E), layer.conv.weight, layer.conv.bias).view(B, H * W, E) + t0
        t = ops.layer_norm(t, m.norm.weight, m.norm.bias)
        return ops.conv3x3(t.view(B, H, W, E), m.conv_after_body.weight, m.conv_after_body.bias) + xf

    def _pixelshuffle_tail(self, img: torch.Tensor) -> torch.Tensor:
        """conv_before_upsample with LeakyReLU 0.01, the PixelShuffle stages, conv_last: [B, H, W, E] token-major -> [B, C, up H, up W]"""
        m = self.module
        B, up = img.shape[0], m.upscale
        c = m.conv_before_upsample[0]
        img = ops.conv3x3(img, c.weight, c.bias, act="lrelu", slope=0.01)
        r = 3 if up == 3 else 2
        for u in range(1 if up == 3 else int(round(math.log2(up)))):
            c = m.upsample[2 * u]
            v = ops.conv3x3(img, c.weight, c.bias)                                                     # [B, h, w, nf r r]
            h_, w_, nf = int(v.shape[1]), int(v.shape[2]), int(v.shape[3]) // (r * r)
            # PixelShuffle(r) in token-major: channel ch r r + ii r + jj of pixel (py, px) -> channel ch of pixel (py r + ii, px r + jj)
            img = v.view(B, h_, w_, nf, r, r).permute(0, 1, 4, 2, 5, 3).reshape(B, h_ * r, w_ * r, nf)
        return ops.conv3x3(img, m.conv_last.weight, m.conv_last.bias).permute(0, 3, 1, 2)


class TrainableSwinIR(TrainableSwin):
    def __init__(self, module: SwinIR, drop_path_rate: float | None = None, generator: torch.Generator | None = None,
                 clamp: bool = False):
        """`drop_path_rate`: None takes the wrapped module's constructor argument.  `clamp`: clamp the output to [0, 1] as Model.forward
        does (models/model.py:48-49)."""
        super().__init__()
        if not isinstance(module, SwinIR):
            raise TypeError(f"TrainableSwinIR wraps a models.SwinIR (got {type(module).__name__})")
        if module.upsampler in ("pixelshuffledirect", "nearest+conv"):
            raise NotImplementedError(f"TrainableSwinIR: upsampler {module.upsampler!r} is not trainable on the MI355X engine "
                                      "(trainable: \"\" and \"pixelshuffle\"); its forward runs through models.SwinIR")
        if module.resi_connection != "1conv":
            raise NotImplementedError(f"TrainableSwinIR: resi_connection {module.resi_connection!r} (\"3conv\") is not trainable on the MI355X "
                                      "engine (trainable: \"1conv\"); its forward runs through models.SwinIR")
        self._wrap(module, drop_path_rate, generator, clamp)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        m = self.module
        self._check_input(x)
        H0, W0 = int(x.shape[2]), int(x.shape[3])
        m.out_size(H0, W0)                                   # the sizes the forward refuses, by the wrapped module's words
        self.last_drop_masks = []
        ph, pw = m._pads(H0, W0)
        up = m.upscale
        mean = self._mean_like(x)
        x = F.pad(x, (0, pw, 0, ph), "reflect") if ph or pw else x
        x = (x - mean) * m.img_range
        img = self._features(x, m.window)
        if m.upsampler == "pixelshuffle":
            y = self._pixelshuffle_tail(img)
        else:
            y = x + ops.conv3x3(img, m.conv_last.weight, m.conv_last.bias).permute(0, 3, 1, 2)
        y = y / m.img_range + mean
        y = y[:, :, :H0 * up, :W0 * up].contiguous()
        return y.clamp(0.0, 1.0) if self.clamp else y
