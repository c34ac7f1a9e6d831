"""Restormer (reference models/transformer/restormer.py:217-406) with the reference constructor signature, parameter names, shapes,
registration order and default initialisation, computing its FORWARD through the MI355X engine (csrc/restormer.hip, exact fp32).

forward(x[B,C,H,W] fp32, CUDA) -> output(...) + x   (reference :368-406; no clamp here, Model.forward clamps)
Forward only: the module works in any grad mode and under torch.inference_mode(), and a backward that reaches it is refused by name.
The submodules below only hold parameters in the reference's layout; the computation is the engine's.
"""
from __future__ import annotations

import torch
from torch import nn

from xmm_superres_denoise.engine import RestormerEngine, XsdError

from .flat_params import FlatParams

MAX_CHANNELS_PER_HEAD = 128     # csrc/restormer.hip: WD_MAXCH (past 64 per head the wide channel-attention kernels run)


class _LayerNormBody(nn.Module):
    def __init__(self, dim: int, with_bias: bool):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        if with_bias:
            self.bias = nn.Parameter(torch.zeros(dim))


class _LayerNorm(nn.Module):            # reference :61-73: `body` is BiasFree_LayerNorm or WithBias_LayerNorm
    def __init__(self, dim: int, layer_norm_type: str):
        super().__init__()
        self.body = _LayerNormBody(dim, layer_norm_type != "BiasFree")


class _FeedForward(nn.Module):          # reference :78-104
    def __init__(self, dim: int, ffn_expansion_factor: float, bias: bool):
        super().__init__()
        hidden = int(dim * ffn_expansion_factor)
        self.project_in = nn.Conv2d(dim, hidden * 2, kernel_size=1, bias=bias)
        self.dwconv = nn.Conv2d(hidden * 2, hidden * 2, kernel_size=3, stride=1, padding=1, groups=hidden * 2, bias=bias)
        self.project_out = nn.Conv2d(hidden, dim, kernel_size=1, bias=bias)


class _Attention(nn.Module):            # reference :109-121 (temperature registered first)
    def __init__(self, dim: int, num_heads: int, bias: bool):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Conv2d(dim, dim * 3, kernel_size=1, bias=bias)
        self.qkv_dwconv = nn.Conv2d(dim * 3, dim * 3, kernel_size=3, stride=1, padding=1, groups=dim * 3, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, kernel_size=1, bias=bias)


class _TransformerBlock(nn.Module):     # reference :156-163
    def __init__(self, dim: int, num_heads: int, ffn_expansion_factor: float, bias: bool, layer_norm_type: str):
        super().__init__()
        self.norm1 = _LayerNorm(dim, layer_norm_type)
        self.attn = _Attention(dim, num_heads, bias)
        self.norm2 = _LayerNorm(dim, layer_norm_type)
        self.ffn = _FeedForward(dim, ffn_expansion_factor, bias)


class _PatchEmbed(nn.Module):           # reference :175-182 (the factory never passes bias: always bias=False)
    def __init__(self, in_c: int, embed_dim: int):
        super().__init__()
        self.proj = nn.Conv2d(in_c, embed_dim, kernel_size=3, stride=1, padding=1, bias=False)


class _Downsample(nn.Module):           # reference :188-199
    def __init__(self, n_feat: int):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat // 2, kernel_size=3, stride=1, padding=1, bias=False), nn.PixelUnshuffle(2))


class _Upsample(nn.Module):             # reference :202-213
    def __init__(self, n_feat: int):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat * 2, kernel_size=3, stride=1, padding=1, bias=False), nn.PixelShuffle(2))


class Restormer(FlatParams, nn.Module):
    ENGINE = RestormerEngine
    NETWORK = "Restormer"

    def __init__(self, inp_channels=3, out_channels=3, dim=48, num_blocks=(4, 6, 6, 8), num_refinement_blocks=4, heads=(1, 2, 4, 8),
                 ffn_expansion_factor=2.66, bias=False, LayerNorm_type="WithBias", dual_pixel_task=False):
        super().__init__()
        # What the engine cannot compute is said HERE, not at the first forward.
        if dual_pixel_task:
            raise ValueError("Restormer: dual_pixel_task=True (dual-pixel defocus deblurring, restormer.py:360-364) is not supported "
                             "by the MI355X engine")
        if inp_channels != out_channels:
            raise ValueError(f"Restormer adds its input to the output (`output(x) + inp_img`, restormer.py:404): inp_channels must equal "
                             f"out_channels (got {inp_channels}, {out_channels})")
        if not 1 <= int(inp_channels) <= 1024:
            raise ValueError(f"inp_channels must be in [1, 1024] (got {inp_channels})")
        if int(dim) < 2 or int(dim) > 1024 or int(dim) % 2:
            raise ValueError(f"dim must be even and in [2, 1024]: Downsample halves it (restormer.py:188; got {dim})")
        num_blocks, heads = [int(n) for n in num_blocks], [int(h) for h in heads]
        if len(num_blocks) != 4 or len(heads) != 4:
            raise ValueError("num_blocks and heads have one entry per level (4)")
        if any(not 0 <= n <= 64 for n in num_blocks) or not 0 <= int(num_refinement_blocks) <= 64:
            raise ValueError("num_blocks / num_refinement_blocks must be in [0, 64]")
        for lvl, chans in ((0, dim), (1, 2 * dim), (2, 4 * dim), (3, 8 * dim), (0, 2 * dim)):
            h = heads[lvl]
            if h < 1 or chans % h or chans // h > MAX_CHANNELS_PER_HEAD:
                raise ValueError(f"heads[{lvl}] = {h} must divide the {chans} channels of its level into at most "
                                 f"{MAX_CHANNELS_PER_HEAD} channels per head")
        if not ffn_expansion_factor > 0 or int(dim * ffn_expansion_factor) < 1:
            raise ValueError(f"ffn_expansion_factor {ffn_expansion_factor} gives no hidden channels")
        # LayerNorm_type: anything but "BiasFree" is WithBias, as in the reference (restormer.py:64-67)
        self.inp_channels, self.out_channels, self.dim = int(inp_channels), int(out_channels), int(dim)
        self.num_blocks, self.num_refinement_blocks, self.heads = num_blocks, int(num_refinement_blocks), heads
        self.ffn_expansion_factor, self.bias, self.LayerNorm_type = float(ffn_expansion_factor), bool(bias), LayerNorm_type

        def level(n, chans, h):
            return nn.Sequential(*[_TransformerBlock(chans, h, ffn_expansion_factor, bias, LayerNorm_type) for _ in range(n)])

        # same construction order as the reference (:232-366) => same parameter order and the same default init under one torch seed
        self.patch_embed = _PatchEmbed(inp_channels, dim)
        self.encoder_level1 = level(num_blocks[0], dim, heads[0])
        self.down1_2 = _Downsample(dim)
        self.encoder_level2 = level(num_blocks[1], dim * 2, heads[1])
        self.down2_3 = _Downsample(dim * 2)
        self.encoder_level3 = level(num_blocks[2], dim * 4, heads[2])
        self.down3_4 = _Downsample(dim * 4)
        self.latent = level(num_blocks[3], dim * 8, heads[3])
        self.up4_3 = _Upsample(dim * 8)
        self.reduce_chan_level3 = nn.Conv2d(dim * 8, dim * 4, kernel_size=1, bias=bias)
        self.decoder_level3 = level(num_blocks[2], dim * 4, heads[2])
        self.up3_2 = _Upsample(dim * 4)
        self.reduce_chan_level2 = nn.Conv2d(dim * 4, dim * 2, kernel_size=1, bias=bias)
        self.decoder_level2 = level(num_blocks[1], dim * 2, heads[1])
        self.up2_1 = _Upsample(dim * 2)
        self.decoder_level1 = level(num_blocks[0], dim * 2, heads[0])
        self.refinement = level(num_refinement_blocks, dim * 2, heads[0])
        self.dual_pixel_task = False
        self.output = nn.Conv2d(dim * 2, out_channels, kernel_size=3, stride=1, padding=1, bias=bias)
        self._init_engine_state()

    def _math_refusal(self, mode: str) -> Exception:
        return ValueError(f"restormer: math mode {mode!r} is not supported: the Restormer engine computes in 'fp32' only")

    def _make_engine(self):
        return RestormerEngine(self.inp_channels, self.out_channels, self.dim, self.num_blocks, self.num_refinement_blocks, self.heads,
                               self.ffn_expansion_factor, self.bias, self.LayerNorm_type == "BiasFree")

    def forward(self, inp_img):
        x = inp_img
        self._check_input(x, self.inp_channels)
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise XsdError(f"Restormer needs H and W divisible by 8 (three PixelUnshuffle(2) levels, restormer.py:188-199); "
                           f"got {x.shape[2]} x {x.shape[3]}")
        return self._forward_only(x, self.out_channels, x.shape[2], x.shape[3])
