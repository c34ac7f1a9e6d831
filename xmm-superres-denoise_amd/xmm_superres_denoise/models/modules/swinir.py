"""SwinIR (reference models/transformer/swinir.py:133-395 with the Swin blocks of modules.py) with the reference constructor signature,
parameter and buffer names, shapes, registration order and default initialisation, computing its FORWARD through the MI355X engine
(csrc/swinir.hip, exact fp32): all four reconstruction heads ("pixelshuffle", "pixelshuffledirect", "nearest+conv", "" = denoising) and
both resi_connection forms ("1conv", "3conv").

forward(x[B,C,H,W] fp32, CUDA) -> [B,C,upscale H,upscale W]   (reference :350-395; no clamp here, Model.forward clamps)
ANY H and W: the engine reflect-pads them to multiples of window_size and crops the output back (check_image_size, :328-333, :395).
The engine computes the EVAL-mode forward: DropPath, Dropout and the attention dropout are identities whatever the module's training
flag, and use_checkpoint changes nothing.  Forward only: the module works in any grad mode and under torch.inference_mode(), and a
backward that reaches it is refused by name.  The submodules below only hold parameters and buffers in the reference's layout; the
computation is the engine's.  The reference has no factory entry and no models.toml name for SwinIR: neither has this package; build
the module directly (or with infer.load_swinir from a checkpoint).
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from xmm_superres_denoise.engine import SwinIREngine, XsdError

from .flat_params import FlatParams
from .swinfir import MAX_HEAD_DIM, MAX_WINDOW, _2tuple, _BasicLayer, _init_weights, _PatchEmbed

UPSAMPLERS = ("pixelshuffle", "pixelshuffledirect", "nearest+conv", "")


def _resi_conv(dim: int, resi_connection: str) -> nn.Module:
    if resi_connection == "1conv":
        return nn.Conv2d(dim, dim, 3, 1, 1)
    # "3conv": to save parameters and memory (swinir.py:89-97, :276-284)
    return nn.Sequential(nn.Conv2d(dim, dim // 4, 3, 1, 1), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                         nn.Conv2d(dim // 4, dim // 4, 1, 1, 0), nn.LeakyReLU(negative_slope=0.2, inplace=True),
                         nn.Conv2d(dim // 4, dim, 3, 1, 1))


class _RSTB(nn.Module):                # swinir.py RSTB (its patch_embed / patch_unembed hold no parameters)
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, qkv_bias, resi_connection):
        super().__init__()
        self.residual_group = _BasicLayer(dim, input_resolution, depth, num_heads, window_size, mlp_ratio, qkv_bias)
        self.conv = _resi_conv(dim, resi_connection)


class _SwinIRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        eng = module._get_engine(x.device)
        module._pack_if_changed()
        return eng.forward(x.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        raise RuntimeError("SwinIR training is not on the MI355X engine: its backward is not implemented (forward only: "
                           "inference, infer.py, validation / test metrics)")


class SwinIR(FlatParams, nn.Module):
    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=[6, 6, 6, 6], num_heads=[6, 6, 6, 6], window_size=7,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.0, upsampler="",
                 resi_connection="1conv"):
        super().__init__()
        # What the engine cannot compute is said HERE, not at the first forward (csrc/swinir.hip: xsd_swinir_create refuses the same).
        if ape:
            raise ValueError("SwinIR: ape=True (absolute position embedding) is not supported by the MI355X engine")
        if upsampler is None:
            upsampler = ""
        if upsampler not in UPSAMPLERS:
            # the reference takes any other string as the denoising head; say so rather than guess
            raise ValueError(f"SwinIR: upsampler {upsampler!r} is not one of {UPSAMPLERS}")
        if resi_connection not in ("1conv", "3conv"):
            raise ValueError(f"SwinIR: resi_connection {resi_connection!r} is not supported (\"1conv\" or \"3conv\")")
        if norm_layer is not nn.LayerNorm:
            raise ValueError("SwinIR: only norm_layer=nn.LayerNorm is supported by the MI355X engine")
        if upscale not in (1, 2, 3, 4, 8):
            raise ValueError(f"SwinIR: upscale {upscale} is not supported. Supported scales: 1, 2^n and 3 (up to 8 here).")
        if upsampler == "nearest+conv" and upscale not in (2, 4):
            raise ValueError(f"SwinIR: upsampler \"nearest+conv\" takes upscale 2 or 4 (got upscale {upscale}: the reference's output size "
                             "would disagree with it)")
        if not 1 <= int(in_chans) <= 64 or not 2 <= int(embed_dim) <= 4096:
            raise ValueError(f"SwinIR: in_chans must be in [1, 64] and embed_dim in [2, 4096] (got {in_chans}, {embed_dim})")
        if resi_connection == "3conv" and int(embed_dim) < 4:
            raise ValueError(f"SwinIR: resi_connection \"3conv\" needs embed_dim >= 4 (got {embed_dim})")
        depths, num_heads = [int(d) for d in depths], [int(h) for h in num_heads]
        if len(depths) > 16 or len(num_heads) < len(depths) or any(not 0 <= d <= 64 for d in depths):
            raise ValueError(f"SwinIR: at most 16 layers of 0..64 blocks, one num_heads entry each (got {depths}, {num_heads})")
        for i, h in enumerate(num_heads[:len(depths)]):
            if h < 1 or embed_dim % h or embed_dim // h > MAX_HEAD_DIM:
                raise ValueError(f"SwinIR: num_heads[{i}] = {h} must divide embed_dim {embed_dim} into at most {MAX_HEAD_DIM} channels "
                                 "per head (head dim)")
        if not mlp_ratio > 0 or int(embed_dim * mlp_ratio) < 1:
            raise ValueError(f"SwinIR: mlp_ratio {mlp_ratio} gives no hidden width")
        if not img_range > 0:
            raise ValueError("SwinIR: img_range must be positive")
        if qk_scale is not None and not qk_scale >= 0:
            raise ValueError(f"SwinIR: qk_scale {qk_scale} is not supported by the MI355X engine (None, or a positive scale)")
        img2, patch2 = _2tuple(img_size), _2tuple(patch_size)
        res = [img2[0] // patch2[0], img2[1] // patch2[1]]
        self.window = min(res) if min(res) <= window_size else window_size     # the effective window (modules.py:236-239)
        if not 1 <= self.window <= MAX_WINDOW:
            raise ValueError(f"SwinIR: an effective window of {self.window} is not supported (1..{MAX_WINDOW}: at most 256 tokens)")
        self.img_size, self.patch_size, self.in_chans, self.embed_dim = img2, patch2, int(in_chans), int(embed_dim)
        self.depths, self.num_heads, self.window_size, self.mlp_ratio = depths, num_heads, int(window_size), float(mlp_ratio)
        self.qkv_bias, self.qk_scale, self.ape, self.patch_norm = bool(qkv_bias), qk_scale, False, bool(patch_norm)
        self.upscale, self.img_range, self.upsampler, self.resi_connection = int(upscale), float(img_range), upsampler, resi_connection
        self.num_layers, self.num_features, self.patches_resolution = len(depths), int(embed_dim), res
        # the fused forward is the eval-mode one and reads none of these; models/modules/swinir_train.py (TrainableSwinIR) does
        self.drop_rate, self.attn_drop_rate, self.drop_path_rate = float(drop_rate), float(attn_drop_rate), float(drop_path_rate)
        if in_chans == 3:
            self.mean = torch.Tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1)
        else:
            self.mean = torch.zeros(1, 1, 1, 1)
        num_feat = 64
        # same construction order as the reference (:201-316) => same parameter order and the same default init under one torch seed
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim, patch_norm)
        self.layers = nn.ModuleList([_RSTB(embed_dim, res, depths[i], num_heads[i], window_size, mlp_ratio, qkv_bias, resi_connection)
                                     for i in range(len(depths))])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = _resi_conv(embed_dim, resi_connection)
        if upsampler == "pixelshuffle":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            ups = []
            if upscale == 3:
                ups += [nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1), nn.PixelShuffle(3)]
            else:
                for _ in range(int(math.log(upscale, 2))):
                    ups += [nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1), nn.PixelShuffle(2)]
            self.upsample = nn.Sequential(*ups)
            self.conv_last = nn.Conv2d(num_feat, in_chans, 3, 1, 1)
        elif upsampler == "pixelshuffledirect":
            self.upsample = nn.Sequential(nn.Conv2d(embed_dim, upscale ** 2 * in_chans, 3, 1, 1), nn.PixelShuffle(upscale))
        elif upsampler == "nearest+conv":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            if upscale == 4:
                self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_last = nn.Conv2d(num_feat, in_chans, 3, 1, 1)
            self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        else:
            self.conv_last = nn.Conv2d(embed_dim, in_chans, 3, 1, 1)
        self.apply(_init_weights)
        self._engine = None
        self._engine_dev = None
        self._flat = None
        self._plist = None
        self._packed_key = None
        self._math = None  # None: the engine's default (fp32)

    def set_math(self, mode: str):
        """Math mode of the linear layers and 3x3 convs (SwinIREngine.set_math): 'fp32' (exact, the default) or 'bf16x6' (strict split).  Kept
        until an engine exists, applied again to the engine a device move creates, and carried by copies and pickles."""
        if mode not in SwinIREngine.MATH:
            raise ValueError(f"SwinIR: math mode {mode!r} is not supported; the modes are {sorted(SwinIREngine.MATH)}"
                             + (" (the fp16 terms of 'f16x3' need a per-tensor scale that these kernels do not publish)" if mode == "f16x3" else ""))
        self._math = mode
        if self._engine is not None:
            self._engine.set_math(mode)
        return self

    def get_math(self) -> str:
        return getattr(self, "_math", None) or "fp32"

    def __getstate__(self):
        st = super().__getstate__()
        st["_packed_key"] = None
        return st

    def _pads(self, H: int, W: int):
        ws = self.window_size
        return (ws - H % ws) % ws, (ws - W % ws) % ws

    def out_size(self, H: int, W: int):
        """(Ho, Wo) of the output for an H x W input, or XsdError for the sizes the forward refuses; needs no device"""
        ph, pw = self._pads(H, W)
        if H < 1 or W < 1 or ph >= H or pw >= W:
            raise XsdError(f"SwinIR: the reflect pad to a multiple of window_size {self.window_size} ({ph} rows, {pw} columns) must be "
                           f"smaller than the image (H = {H}, W = {W}), as in F.pad")
        Hp, Wp = H + ph, W + pw
        if Hp % self.window or Wp % self.window:
            raise XsdError(f"SwinIR: the padded size {Hp} x {Wp} (multiples of window_size {self.window_size}) is no multiple of the "
                           f"effective window {self.window}, which img_size // patch_size clamped (window_partition)")
        f = 1 if self.upsampler == "" else self.upscale
        return min(H * self.upscale, Hp * f), min(W * self.upscale, Wp * f)

    def _get_engine(self, device):
        if not torch.device(device).type == "cuda":
            raise XsdError("the MI355X engine needs CUDA(HIP) tensors; there is no CPU fallback")
        flat = self.flatten_parameters()
        if flat.device != torch.device(device):
            raise XsdError(f"module parameters are on {flat.device} but the input is on {device}")
        if self._engine is None or self._engine_dev != flat.device:
            with torch.cuda.device(flat.device):
                self._engine = SwinIREngine(self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.depths, self.num_heads,
                                            self.window_size, self.mlp_ratio, self.qkv_bias, self.qk_scale, self.ape, self.patch_norm,
                                            self.upscale, self.img_range, self.upsampler, self.resi_connection)
            self._engine_dev = flat.device
            self._packed_key = None
            if getattr(self, "_math", None) is not None:
                self._engine.set_math(self._math)
        return self._engine

    def _pack_if_changed(self):
        """Re-pack after any parameter update torch knows of (optimizer step, load_state_dict, in-place edits: the version counters
        of the parameters and of the flat buffer) or a new flat buffer."""
        key = (self._flat.data_ptr(), self._param_version())
        if key != self._packed_key:
            self._engine.pack(self._flat)
            self._packed_key = key

    def forward(self, x):
        if x.dtype != torch.float32:
            raise XsdError(f"input must be float32 (got {x.dtype})")
        if x.dim() != 4 or x.shape[1] != self.in_chans:
            raise XsdError(f"input must be [B,{self.in_chans},H,W] (got {tuple(x.shape)})")
        Ho, Wo = self.out_size(int(x.shape[2]), int(x.shape[3]))
        self._get_engine(x.device)
        if x.shape[0] == 0:      # an empty batch answers like torch's convs: empty output, no launch
            return x.new_empty((0, self.in_chans, Ho, Wo))
        return _SwinIRFn.apply(self, x, *self._plist)
