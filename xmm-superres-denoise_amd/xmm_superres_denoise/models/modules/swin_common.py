"""What SwinFIR, HAT and SwinIR share: the Swin blocks of the reference's modules.py as parameter holders, and SwinFamily, the base of
the three modules: the constructor checks whose words differ only in the network's name, the constructor arguments as attributes, the
`mean` tensor and the pixel-shuffle head.  Checks that a network words in its own way stay in its module."""
from __future__ import annotations

import math

import torch
from torch import nn

from .flat_params import FlatParams

MAX_WINDOW = 16          # csrc/swinfir.hip: sw_attn_kernel takes at most 8 tiles of 32 tokens per window
MAX_HEAD_DIM = 32        # one 32-column MFMA tile per head


def _2tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _init_weights(m):
    # reference tools.py init_weights, applied by SwinFIR.__init__ to every submodule; timm's trunc_normal_ is the same truncated
    # normal draw as torch.nn.init.trunc_normal_ (bounds +-2, std 0.02)
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


def relative_position_index(ws: int) -> torch.Tensor:
    """[ws^2, ws^2] index into the (2 ws - 1)^2 bias table: (dy + ws - 1) (2 ws - 1) + (dx + ws - 1) for tokens i, j"""
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous() + (ws - 1)
    return rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]


def shift_mask(h: int, w: int, ws: int, shift: int) -> torch.Tensor:
    """[nW, ws^2, ws^2]: 0 between tokens of the same region of the rolled image, -100 otherwise (the reference's attn_mask)"""
    def region(n):
        r = torch.zeros(n)
        r[n - ws:n - shift] = 1
        r[n - shift:] = 2
        return r
    ids = (3 * region(h)[:, None] + region(w)[None, :])
    win = ids.view(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    d = win[:, None, :] - win[:, :, None]
    return torch.where(d != 0, torch.tensor(-100.0), torch.tensor(0.0))


class _Mlp(nn.Module):                 # modules.py Mlp
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)


class _WindowAttention(nn.Module):     # modules.py WindowAttention: table, index buffer, qkv, proj; the table drawn last
    def __init__(self, dim: int, ws: int, num_heads: int, qkv_bias: bool):
        super().__init__()
        self.num_heads = num_heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(ws))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)


class _SwinBlock(nn.Module):           # modules.py SwinTransformerBlock
    def __init__(self, dim, input_resolution, num_heads, window_size, shift_size, mlp_ratio, qkv_bias):
        super().__init__()
        self.window_size, self.shift_size = window_size, shift_size
        if min(input_resolution) <= window_size:
            self.shift_size, self.window_size = 0, min(input_resolution)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, self.window_size, num_heads, qkv_bias)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        mask = shift_mask(input_resolution[0], input_resolution[1], self.window_size, self.shift_size) if self.shift_size > 0 else None
        self.register_buffer("attn_mask", mask)


class _BasicLayer(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, qkv_bias):
        super().__init__()
        self.blocks = nn.ModuleList([_SwinBlock(dim, input_resolution, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2,
                                                mlp_ratio, qkv_bias) for i in range(depth)])


class _PatchEmbed(nn.Module):
    def __init__(self, dim: int, patch_norm: bool):
        super().__init__()
        self.norm = nn.LayerNorm(dim) if patch_norm else None


def conv_before_upsample(embed_dim: int, num_feat: int) -> nn.Module:
    return nn.Sequential(nn.Conv2d(embed_dim, num_feat, 3, 1, 1), nn.LeakyReLU(inplace=True))


class SwinFamily(FlatParams, nn.Module):
    """Base of SwinFIR, HAT and SwinIR.  A subclass names NETWORK, ENGINE and the RGB triple of its `mean`."""

    RGB_MEAN = (0.4488, 0.4371, 0.4040)

    def _head_refusal(self, i: int, h: int, embed_dim: int):
        """what is wrong with num_heads[i] = h, or None"""
        if h < 1 or embed_dim % h or embed_dim // h > MAX_HEAD_DIM:
            return (f"{self.NETWORK}: num_heads[{i}] = {h} must divide embed_dim {embed_dim} into at most {MAX_HEAD_DIM} channels "
                    "per head")

    def _swin_args(self, img_size, patch_size, in_chans, embed_dim, depths, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale,
                   drop_rate, attn_drop_rate, drop_path_rate, norm_layer, ape, patch_norm, upscale, img_range, upsampler, resi_connection):
        """The checks the three networks word alike, then the constructor arguments as attributes and `mean`.  What the engine cannot
        compute is said in the constructor, not at the first forward.  Returns img_size // patch_size."""
        name = self.NETWORK
        if ape:
            raise ValueError(f"{name}: ape=True (absolute position embedding) is not supported by the MI355X engine")
        if norm_layer is not nn.LayerNorm:
            raise ValueError(f"{name}: only norm_layer=nn.LayerNorm is supported by the MI355X engine")
        if not 1 <= int(in_chans) <= 64 or not 2 <= int(embed_dim) <= 4096:
            raise ValueError(f"{name}: in_chans must be in [1, 64] and embed_dim in [2, 4096] (got {in_chans}, {embed_dim})")
        depths, num_heads = [int(d) for d in depths], [int(h) for h in num_heads]
        if len(depths) > 16 or len(num_heads) < len(depths) or any(not 0 <= d <= 64 for d in depths):
            raise ValueError(f"{name}: at most 16 layers of 0..64 blocks, one num_heads entry each (got {depths}, {num_heads})")
        for i, h in enumerate(num_heads[:len(depths)]):
            refusal = self._head_refusal(i, h, embed_dim)
            if refusal:
                raise ValueError(refusal)
        if not mlp_ratio > 0 or int(embed_dim * mlp_ratio) < 1:
            raise ValueError(f"{name}: mlp_ratio {mlp_ratio} gives no hidden width")
        if not img_range > 0:
            raise ValueError(f"{name}: img_range must be positive")
        if qk_scale is not None and not qk_scale >= 0:
            # the reference would use a negative scale as given; the engine takes None / 0 (head_dim^-0.5) or a positive one
            raise ValueError(f"{name}: qk_scale {qk_scale} is not supported by the MI355X engine (None, or a positive scale)")
        img2, patch2 = _2tuple(img_size), _2tuple(patch_size)
        res = [img2[0] // patch2[0], img2[1] // patch2[1]]
        self.img_size, self.patch_size, self.in_chans, self.embed_dim = img2, patch2, int(in_chans), int(embed_dim)
        self.depths, self.num_heads, self.window_size, self.mlp_ratio = depths, num_heads, int(window_size), float(mlp_ratio)
        self.qkv_bias, self.qk_scale, self.ape, self.patch_norm = bool(qkv_bias), qk_scale, False, bool(patch_norm)
        self.upscale, self.img_range, self.upsampler, self.resi_connection = int(upscale), float(img_range), upsampler, resi_connection
        self.num_layers, self.num_features, self.patches_resolution = len(depths), int(embed_dim), res
        # the fused forward is the eval-mode one and reads none of these; the Trainable* wrappers (swinir_train.py) do
        self.drop_rate, self.attn_drop_rate, self.drop_path_rate = float(drop_rate), float(attn_drop_rate), float(drop_path_rate)
        self.mean = torch.Tensor(self.RGB_MEAN).view(1, 3, 1, 1) if in_chans == 3 else torch.zeros(1, 1, 1, 1)
        return res

    def _effective_window(self, res, window_size):
        """the window the blocks use (modules.py:236-239 clamps it to the token grid)"""
        self.window = min(res) if min(res) <= window_size else window_size
        if not 1 <= self.window <= MAX_WINDOW:
            raise ValueError(f"{self.NETWORK}: an effective window of {self.window} is not supported (1..{MAX_WINDOW}: at most 256 tokens)")

    def _pixelshuffle_head(self, embed_dim, in_chans, upscale, num_feat=64):
        """conv_before_upsample, upsample, conv_last in the reference's construction order (=> its parameter order and default init)"""
        self.conv_before_upsample = conv_before_upsample(embed_dim, num_feat)
        ups = []
        if upscale == 3:
            ups += [nn.Conv2d(num_feat, 9 * num_feat, 3, 1, 1), nn.PixelShuffle(3)]
        else:
            for _ in range(int(math.log(upscale, 2))):
                ups += [nn.Conv2d(num_feat, 4 * num_feat, 3, 1, 1), nn.PixelShuffle(2)]
        self.upsample = nn.Sequential(*ups)
        self.conv_last = nn.Conv2d(num_feat, in_chans, 3, 1, 1)
