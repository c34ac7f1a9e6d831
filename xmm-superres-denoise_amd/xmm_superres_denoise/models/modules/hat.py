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

import torch
from torch import nn

from xmm_superres_denoise.engine import HATEngine, XsdError

from .swin_common import MAX_HEAD_DIM, MAX_WINDOW, SwinFamily, _init_weights, _Mlp, _PatchEmbed, relative_position_index

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


class HAT(SwinFamily):
    ENGINE = HATEngine
    NETWORK = "HAT"

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 use_checkpoint=False, upscale=2, img_range=1.0, upsampler="", resi_connection="1conv"):
        super().__init__()
        # What the engine cannot compute is said HERE, not at the first forward.
        if upsampler != "pixelshuffle":
            raise ValueError(f"HAT: upsampler {upsampler!r} is not supported by the MI355X engine (only \"pixelshuffle\"; with any other "
                             "value the reference's forward returns its input)")
        if resi_connection not in ("1conv", "identity"):
            raise ValueError(f"HAT: resi_connection {resi_connection!r} is not supported (only \"1conv\" and \"identity\": the reference's "
                             "HAT has no other branch)")
        if upscale not in (2, 3, 4, 8):
            raise ValueError(f"HAT: scale {upscale} is not supported. Supported scales: 2^n and 3 (up to 8 here).")
        res = self._swin_args(img_size, patch_size, in_chans, embed_dim, depths, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale,
                              drop_rate, attn_drop_rate, drop_path_rate, norm_layer, ape, patch_norm, upscale, img_range, upsampler,
                              resi_connection)
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
        if min(res) < window_size:
            raise ValueError(f"HAT: img_size // patch_size = {min(res)} is smaller than window_size {window_size}: the reference's HAB clamps "
                             "its window but the relative position index does not follow, and its forward fails")
        self.window = int(window_size)
        self.shift_size, self.overlap_ratio = int(window_size) // 2, overlap_ratio
        self.compress_ratio, self.squeeze_factor, self.conv_scale = int(compress_ratio), int(squeeze_factor), float(conv_scale)
        self.register_buffer("relative_position_index_SA", relative_position_index(self.window))
        self.register_buffer("relative_position_index_OCA", relative_position_index_oca(self.window, self.window + ext))
        # same construction order as the reference (:694-785) => same parameter order and the same default init under one torch seed
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim, patch_norm)
        self.layers = nn.ModuleList([_RHAG(embed_dim, res, self.depths[i], self.num_heads[i], self.window, self.compress_ratio,
                                           self.squeeze_factor, self.conv_scale, overlap_ratio, mlp_ratio, qkv_bias, resi_connection)
                                     for i in range(len(self.depths))])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1) if resi_connection == "1conv" else nn.Identity()
        self._pixelshuffle_head(embed_dim, in_chans, upscale)
        self.apply(_init_weights)
        self._init_engine_state()

    def _head_refusal(self, i: int, h: int, embed_dim: int):
        if h < 1 or embed_dim % h:
            return f"HAT: num_heads[{i}] = {h} does not divide embed_dim {embed_dim}"
        if embed_dim // h > MAX_HEAD_DIM:
            return (f"HAT: num_heads[{i}] = {h} gives a head dim of {embed_dim // h}; the engine takes at most {MAX_HEAD_DIM} "
                    "channels per head")

    def _make_engine(self):
        return HATEngine(self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.depths, self.num_heads, self.window_size,
                         self.compress_ratio, self.squeeze_factor, self.conv_scale, self.overlap_ratio, self.mlp_ratio, self.qkv_bias,
                         self.qk_scale, self.ape, self.patch_norm, self.upscale, self.img_range, self.upsampler, self.resi_connection)

    def forward(self, x):
        self._check_input(x, self.in_chans)
        H, W = int(x.shape[2]), int(x.shape[3])
        if H % self.window or W % self.window:
            raise XsdError(f"HAT needs H and W that are multiples of the window size {self.window} (window_partition; the reference does "
                           f"not pad); got {H} x {W}")
        return self._forward_only(x, self.in_chans, H * self.upscale, W * self.upscale)
