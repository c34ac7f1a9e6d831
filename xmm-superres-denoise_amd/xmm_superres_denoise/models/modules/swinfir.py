"""SwinFIR (reference models/transformer/swinfir.py:120-441 with the Swin blocks of modules.py) with the reference constructor signature,
parameter and buffer names, shapes, registration order and default initialisation, computing its FORWARD through the MI355X engine
(csrc/swinfir.hip, exact fp32).

forward(x[B,C,H,W] fp32, CUDA) -> [B,C,upscale H,upscale W]   (reference :420-441; no clamp here, Model.forward clamps)
The engine computes the EVAL-mode forward: DropPath, Dropout and the attention dropout are identities whatever the module's training
flag, and use_checkpoint (a memory policy of the reference's training) changes nothing.  Forward only: the module works in any grad mode
and under torch.inference_mode(), and a backward that reaches it is refused by name.  The submodules below only hold parameters and
buffers in the reference's layout; the computation is the engine's.
"""
from __future__ import annotations

from torch import nn

from xmm_superres_denoise.engine import SwinFIREngine, XsdError, fft_size_supported

from .swin_common import SwinFamily, _BasicLayer, _init_weights, _PatchEmbed


class _ResB(nn.Module):                # swinfir.py ResB
    def __init__(self, dim: int):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(dim, dim, 3, 1, 1), nn.LeakyReLU(0.2, inplace=True), nn.Conv2d(dim, dim, 3, 1, 1))


class _FourierUnit(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv_layer = nn.Conv2d(c * 2, c * 2, 1, 1, 0)
        self.relu = nn.LeakyReLU(0.2, inplace=True)


class _SpectralTransform(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(dim, dim // 2, 1, 1, 0), nn.LeakyReLU(0.2, inplace=True))
        self.fu = _FourierUnit(dim // 2)
        self.conv2 = nn.Conv2d(dim // 2, dim, 1, 1, 0)


class _SFB(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.S = _ResB(dim)
        self.F = _SpectralTransform(dim)
        self.fusion = nn.Conv2d(dim * 2, dim, 1, 1, 0)


class _RSTB(nn.Module):                # swinfir.py RSTB (its patch_embed / patch_unembed hold no parameters)
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio, qkv_bias, resi_connection):
        super().__init__()
        self.residual_group = _BasicLayer(dim, input_resolution, depth, num_heads, window_size, mlp_ratio, qkv_bias)
        self.conv = _SFB(dim) if resi_connection == "SFB" else nn.Conv2d(dim, dim, 3, 1, 1)


class SwinFIR(SwinFamily):
    ENGINE = SwinFIREngine
    NETWORK = "SwinFIR"
    RGB_MEAN = (0.3014, 0.3152, 0.3094)

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.0, upsampler="",
                 resi_connection="SFB"):
        super().__init__()
        # What the engine cannot compute is said HERE, not at the first forward.
        if upsampler != "pixelshuffle":
            raise ValueError(f"SwinFIR: upsampler {upsampler!r} is not supported by the MI355X engine (only \"pixelshuffle\", the XMM "
                             "configuration's)")
        if resi_connection not in ("SFB", "1conv"):
            raise ValueError(f"SwinFIR: resi_connection {resi_connection!r} is not supported by the MI355X engine (only \"SFB\" and "
                             "\"1conv\")")
        if upscale not in (2, 3, 4, 8):
            raise ValueError(f"SwinFIR: scale {upscale} is not supported. Supported scales: 2^n and 3 (up to 8 here).")
        res = self._swin_args(img_size, patch_size, in_chans, embed_dim, depths, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale,
                              drop_rate, attn_drop_rate, drop_path_rate, norm_layer, ape, patch_norm, upscale, img_range, upsampler,
                              resi_connection)
        self._effective_window(res, window_size)
        # same construction order as the reference (:315-401) => same parameter order and the same default init under one torch seed
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim, patch_norm)
        self.layers = nn.ModuleList([_RSTB(embed_dim, res, self.depths[i], self.num_heads[i], window_size, mlp_ratio, qkv_bias,
                                           resi_connection) for i in range(len(self.depths))])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        self._pixelshuffle_head(embed_dim, in_chans, upscale)
        self.apply(_init_weights)
        self._init_engine_state()

    def _make_engine(self):
        return SwinFIREngine(self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.depths, self.num_heads, self.window_size,
                             self.mlp_ratio, self.qkv_bias, self.qk_scale, self.ape, self.patch_norm, self.upscale, self.img_range,
                             self.upsampler, self.resi_connection)

    def forward(self, x):
        self._check_input(x, self.in_chans)
        H, W = int(x.shape[2]), int(x.shape[3])
        if H % self.window or W % self.window:
            raise XsdError(f"SwinFIR needs H and W that are multiples of the window size {self.window} (window_partition, "
                           f"modules.py); got {H} x {W}")
        if self.resi_connection == "SFB":
            for n in (H, W):
                if not fft_size_supported(n):
                    raise XsdError(f"SwinFIR: FFT size {n} is not supported (the FourierUnit needs H and W of at most 4096 whose prime "
                                   f"factors are all <= 13); got {H} x {W}")
        return self._forward_only(x, self.in_chans, H * self.upscale, W * self.upscale)
