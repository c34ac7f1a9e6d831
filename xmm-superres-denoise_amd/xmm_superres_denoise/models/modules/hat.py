"""HAT (reference models/transformer/hat.py:10-913) with the reference constructor signature, parameter and buffer names, shapes,
registration order and default initialisation, computing its FORWARD through the MI355X engine (csrc/hat.hip, exact fp32).

forward(x[B,C,H,W] fp32, CUDA) -> [B,C,upscale H,upscale W]   (reference :900-913; no clamp here, Model.forward clamps)
The engine computes the EVAL-mode forward: DropPath, Dropout and the attention dropout are identities whatever the module's training
flag, and use_checkpoint (a memory policy of the reference's training) changes nothing.  Forward only: the module works in any grad mode
and under torch.inference_mode(), and a backward that reaches it is refused by name.  The submodules below only hold parameters and
buffers in the reference's layout; the computation is the engine's.  Like the reference, the module stores no attn_mask: the shift mask is
the one of the run-time size (reference :836-865, :880), computed inside the attention kernel.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from xmm_superres_denoise.engine import HATEngine, XsdError

from .flat_params import FlatParams
from .swinfir import MAX_HEAD_DIM, MAX_WINDOW, _2tuple, _init_weights, _Mlp, _PatchEmbed, relative_position_index

MAX_OVERLAP_WINDOW = 32  # csrc/hat.hip: OC_MAX_OW, at most 1024 keys per window


def relative_position_index_oca(ws: int, ow: int) -> torch.Tensor:
    """[ws^2, ow^2] index into the (ws + ow - 1)^2 bias table of an OCAB, as the reference computes it (:805-834): (dy + ws - ow + 1)
    (ws + ow - 1) + (dx + ws - ow + 1) for the offset (dy, dx) of key j of the overlapping window from query i.  The shift is the
    reference's: part of the entries are negative and index the table from its end."""
    q = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    k = torch.stack(torch.meshgrid(torch.arange(ow), torch.arange(ow), indexing="ij")).flatten(1)
    rel = (k[:, None, :] - q[:, :, None]).permute(1, 2, 0).contiguous() + (ws - ow + 1)
    return rel[:, :, 0] * (ws + ow - 1) + rel[:, :, 1]


class _WindowAttention(nn.Module):     # hat.py WindowAttention: table, qkv, proj; the table drawn last; the index lives in HAT
    def __init__(self, dim: int, ws: int, num_heads: int, qkv_bias: bool):
        super().__init__()
        self.num_heads = num_heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)


class _ChannelAttention(nn.Module):    # hat.py ChannelAttention: pool, conv1x1, ReLU, conv1x1, Sigmoid
    def __init__(self, num_feat: int, squeeze_factor: int):
        super().__init__()
        self.attention = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(num_feat, num_feat // squeeze_factor, 1, padding=0),
                                       nn.ReLU(inplace=True), nn.Conv2d(num_feat // squeeze_factor, num_feat, 1, padding=0), nn.Sigmoid())


class _CAB(nn.Module):
    def __init__(self, num_feat: int, compress_ratio: int, squeeze_factor: int):
        super().__init__()
        self.cab = nn.Sequential(nn.Conv2d(num_feat, num_feat // compress_ratio, 3, 1, 1), nn.GELU(),
                                 nn.Conv2d(num_feat // compress_ratio, num_feat, 3, 1, 1), _ChannelAttention(num_feat, squeeze_factor))


class _HAB(nn.Module):                 # hat.py HAB
    def __init__(self, dim, input_resolution, num_heads, window_size, shift_size, compress_ratio, squeeze_factor, conv_scale, mlp_ratio,
                 qkv_bias):
        super().__init__()
        self.window_size, self.shift_size, self.conv_scale = window_size, shift_size, conv_scale
        if min(input_resolution) <= window_size:
            self.shift_size, self.window_size = 0, min(input_resolution)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, self.window_size, num_heads, qkv_bias)
        self.conv_block = _CAB(dim, compress_ratio, squeeze_factor)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _OCAB(nn.Module):                # hat.py OCAB: norm1, qkv, the table (drawn before proj is built), proj, norm2, mlp
    def __init__(self, dim, window_size, overlap_ratio, num_heads, qkv_bias, mlp_ratio):
        super().__init__()
        self.window_size, self.num_heads = window_size, num_heads
        self.overlap_win_size = int(window_size * overlap_ratio) + window_size
        self.norm1 = nn.LayerNorm(dim)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((window_size + self.overlap_win_size - 1) ** 2, num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _AttenBlocks(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, compress_ratio, squeeze_factor, conv_scale, overlap_ratio,
                 mlp_ratio, qkv_bias):
        super().__init__()
        self.blocks = nn.ModuleList([_HAB(dim, input_resolution, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2,
                                          compress_ratio, squeeze_factor, conv_scale, mlp_ratio, qkv_bias) for i in range(depth)])
        self.overlap_attn = _OCAB(dim, window_size, overlap_ratio, num_heads, qkv_bias, mlp_ratio)


class _RHAG(nn.Module):                # hat.py RHAG (its patch_embed / patch_unembed hold no parameters)
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, compress_ratio, squeeze_factor, conv_scale, overlap_ratio,
                 mlp_ratio, qkv_bias, resi_connection):
        super().__init__()
        self.residual_group = _AttenBlocks(dim, input_resolution, depth, num_heads, window_size, compress_ratio, squeeze_factor,
                                           conv_scale, overlap_ratio, mlp_ratio, qkv_bias)
        self.conv = nn.Conv2d(dim, dim, 3, 1, 1) if resi_connection == "1conv" else nn.Identity()


class _HATFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        eng = module._get_engine(x.device)
        module._pack_if_changed()
        return eng.forward(x.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        raise RuntimeError("HAT training is not on the MI355X engine: its backward is not implemented (forward only: "
                           "inference, infer.py, validation / test metrics)")


class HAT(FlatParams, nn.Module):
    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 use_checkpoint=False, upscale=2, img_range=1.0, upsampler="", resi_connection="1conv"):
        super().__init__()
        # What the engine cannot compute is said HERE, not at the first forward.
        if ape:
            raise ValueError("HAT: ape=True (absolute position embedding) is not supported by the MI355X engine")
        if upsampler != "pixelshuffle":
            raise ValueError(f"HAT: upsampler {upsampler!r} is not supported by the MI355X engine (only \"pixelshuffle\"; with any other "
                             "value the reference's forward returns its input)")
        if resi_connection not in ("1conv", "identity"):
            raise ValueError(f"HAT: resi_connection {resi_connection!r} is not supported (only \"1conv\" and \"identity\": the reference's "
                             "HAT has no other branch)")
        if norm_layer is not nn.LayerNorm:
            raise ValueError("HAT: only norm_layer=nn.LayerNorm is supported by the MI355X engine")
        if upscale not in (2, 3, 4, 8):
            raise ValueError(f"HAT: scale {upscale} is not supported. Supported scales: 2^n and 3 (up to 8 here).")
        if not 1 <= int(in_chans) <= 64 or not 2 <= int(embed_dim) <= 4096:
            raise ValueError(f"HAT: in_chans must be in [1, 64] and embed_dim in [2, 4096] (got {in_chans}, {embed_dim})")
        depths, num_heads = [int(d) for d in depths], [int(h) for h in num_heads]
        if len(depths) > 16 or len(num_heads) < len(depths) or any(not 0 <= d <= 64 for d in depths):
            raise ValueError(f"HAT: at most 16 layers of 0..64 blocks, one num_heads entry each (got {depths}, {num_heads})")
        for i, h in enumerate(num_heads[:len(depths)]):
            if h < 1 or embed_dim % h:
                raise ValueError(f"HAT: num_heads[{i}] = {h} does not divide embed_dim {embed_dim}")
            if embed_dim // h > MAX_HEAD_DIM:
                raise ValueError(f"HAT: num_heads[{i}] = {h} gives a head dim of {embed_dim // h}; the engine takes at most {MAX_HEAD_DIM} "
                                 "channels per head")
        if not mlp_ratio > 0 or int(embed_dim * mlp_ratio) < 1:
            raise ValueError(f"HAT: mlp_ratio {mlp_ratio} gives no hidden width")
        if not img_range > 0:
            raise ValueError("HAT: img_range must be positive")
        if qk_scale is not None and not qk_scale >= 0:
            # the reference would use a negative scale as given; the engine takes None / 0 (head_dim^-0.5) or a positive one
            raise ValueError(f"HAT: qk_scale {qk_scale} is not supported by the MI355X engine (None, or a positive scale)")
        if not 1 <= int(window_size) <= MAX_WINDOW:
            raise ValueError(f"HAT: window_size {window_size} is not supported (1..{MAX_WINDOW}: at most 256 tokens per window)")
        if not overlap_ratio >= 0:
            raise ValueError(f"HAT: overlap_ratio {overlap_ratio} must not be negative")
        ext = int(window_size * overlap_ratio)
        if ext % 2:
            raise ValueError(f"HAT: int(window_size * overlap_ratio) = {ext} is odd: the reference's unfold (padding {ext} // 2) then yields "
                             "the wrong number of windows and its forward fails")
        if window_size + ext > MAX_OVERLAP_WINDOW:
            raise ValueError(f"HAT: an overlap window of {window_size + ext} is not supported by the MI355X engine (at most "
                             f"{MAX_OVERLAP_WINDOW})")
        if window_size * (2 * window_size + ext) >= (2 * window_size + ext - 1) ** 2:
            raise ValueError(f"HAT: window_size {window_size} with an overlap window of {window_size + ext} indexes past the OCAB's bias "
                             "table in the reference")
        if int(compress_ratio) < 1 or embed_dim // int(compress_ratio) < 1:
            raise ValueError(f"HAT: embed_dim // compress_ratio = {embed_dim} // {compress_ratio} leaves the CAB no channels")
        if int(squeeze_factor) < 1 or embed_dim // int(squeeze_factor) < 1:
            raise ValueError(f"HAT: embed_dim // squeeze_factor = {embed_dim} // {squeeze_factor} leaves the channel attention no channels")
        img2, patch2 = _2tuple(img_size), _2tuple(patch_size)
        res = [img2[0] // patch2[0], img2[1] // patch2[1]]
        if min(res) < window_size:
            raise ValueError(f"HAT: img_size // patch_size = {min(res)} is smaller than window_size {window_size}: the reference's HAB clamps "
                             "its window but the relative position index does not follow, and its forward fails")
        self.window = int(window_size)
        self.img_size, self.patch_size, self.in_chans, self.embed_dim = img2, patch2, int(in_chans), int(embed_dim)
        self.depths, self.num_heads, self.window_size, self.mlp_ratio = depths, num_heads, int(window_size), float(mlp_ratio)
        self.shift_size, self.overlap_ratio = int(window_size) // 2, overlap_ratio
        self.compress_ratio, self.squeeze_factor, self.conv_scale = int(compress_ratio), int(squeeze_factor), float(conv_scale)
        self.qkv_bias, self.qk_scale, self.ape, self.patch_norm = bool(qkv_bias), qk_scale, False, bool(patch_norm)
        self.upscale, self.img_range, self.upsampler, self.resi_connection = int(upscale), float(img_range), upsampler, resi_connection
        self.num_layers, self.num_features, self.patches_resolution = len(depths), int(embed_dim), res
        if in_chans == 3:
            self.mean = torch.Tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1)
        else:
            self.mean = torch.zeros(1, 1, 1, 1)
        num_feat = 64
        self.register_buffer("relative_position_index_SA", relative_position_index(self.window))
        self.register_buffer("relative_position_index_OCA", relative_position_index_oca(self.window, self.window + ext))
        # same construction order as the reference (:694-785) => same parameter order and the same default init under one torch seed
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim, patch_norm)
        self.layers = nn.ModuleList([_RHAG(embed_dim, res, depths[i], num_heads[i], self.window, self.compress_ratio, self.squeeze_factor,
                                           self.conv_scale, overlap_ratio, mlp_ratio, qkv_bias, resi_connection)
                                     for i in range(len(depths))])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1) if resi_connection == "1conv" else nn.Identity()
        self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))
        ups = []
        if upscale == 3:
            ups += [nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1), nn.PixelShuffle(3)]
        else:
            for _ in range(int(math.log(upscale, 2))):
                ups += [nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1), nn.PixelShuffle(2)]
        self.upsample = nn.Sequential(*ups)
        self.conv_last = nn.Conv2d(num_feat, in_chans, 3, 1, 1)
        self.apply(_init_weights)
        self._engine = None
        self._engine_dev = None
        self._flat = None
        self._plist = None
        self._packed_key = None
        self._math = None  # None: the engine's default (fp32)

    def set_math(self, mode: str):
        """Math mode of the linear layers and 3x3 convs (HATEngine.set_math): 'fp32' (exact, the default) or 'bf16x6' (strict split).  Kept
        until an engine exists, applied again to the engine a device move creates, and carried by copies and pickles."""
        if mode not in HATEngine.MATH:
            raise ValueError(f"HAT: math mode {mode!r} is not supported; the modes are {sorted(HATEngine.MATH)}"
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

    def _get_engine(self, device):
        if not torch.device(device).type == "cuda":
            raise XsdError("the MI355X engine needs CUDA(HIP) tensors; there is no CPU fallback")
        flat = self.flatten_parameters()
        if flat.device != torch.device(device):
            raise XsdError(f"module parameters are on {flat.device} but the input is on {device}")
        if self._engine is None or self._engine_dev != flat.device:
            with torch.cuda.device(flat.device):
                self._engine = HATEngine(self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.depths, self.num_heads,
                                         self.window_size, self.compress_ratio, self.squeeze_factor, self.conv_scale, self.overlap_ratio,
                                         self.mlp_ratio, self.qkv_bias, self.qk_scale, self.ape, self.patch_norm, self.upscale,
                                         self.img_range, self.upsampler, self.resi_connection)
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
        H, W = int(x.shape[2]), int(x.shape[3])
        if H % self.window or W % self.window:
            raise XsdError(f"HAT needs H and W that are multiples of the window size {self.window} (window_partition; the reference does "
                           f"not pad); got {H} x {W}")
        self._get_engine(x.device)
        s = self.upscale
        if x.shape[0] == 0:      # an empty batch answers like torch's convs: empty output, no launch
            return x.new_empty((0, self.in_chans, H * s, W * s))
        return _HATFn.apply(self, x, *self._plist)
