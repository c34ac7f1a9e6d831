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

from torch import nn

from xmm_superres_denoise.engine import SwinIREngine, XsdError

from .swin_common import SwinFamily, _BasicLayer, _init_weights, _PatchEmbed, conv_before_upsample

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


class SwinIR(SwinFamily):
    ENGINE = SwinIREngine
    NETWORK = "SwinIR"

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=[6, 6, 6, 6], num_heads=[6, 6, 6, 6], window_size=7,
                 mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.0, upsampler="",
                 resi_connection="1conv"):
        super().__init__()
        # What the engine cannot compute is said HERE, not at the first forward (csrc/swinir.hip: xsd_swinir_create refuses the same).
        if upsampler is None:
            upsampler = ""
        if upsampler not in UPSAMPLERS:
            # the reference takes any other string as the denoising head; say so rather than guess
            raise ValueError(f"SwinIR: upsampler {upsampler!r} is not one of {UPSAMPLERS}")
        if resi_connection not in ("1conv", "3conv"):
            raise ValueError(f"SwinIR: resi_connection {resi_connection!r} is not supported (\"1conv\" or \"3conv\")")
        if upscale not in (1, 2, 3, 4, 8):
            raise ValueError(f"SwinIR: upscale {upscale} is not supported. Supported scales: 1, 2^n and 3 (up to 8 here).")
        if upsampler == "nearest+conv" and upscale not in (2, 4):
            raise ValueError(f"SwinIR: upsampler \"nearest+conv\" takes upscale 2 or 4 (got upscale {upscale}: the reference's output size "
                             "would disagree with it)")
        res = self._swin_args(img_size, patch_size, in_chans, embed_dim, depths, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale,
                              drop_rate, attn_drop_rate, drop_path_rate, norm_layer, ape, patch_norm, upscale, img_range, upsampler,
                              resi_connection)
        if resi_connection == "3conv" and int(embed_dim) < 4:
            raise ValueError(f"SwinIR: resi_connection \"3conv\" needs embed_dim >= 4 (got {embed_dim})")
        self._effective_window(res, window_size)
        num_feat = 64
        # same construction order as the reference (:201-316) => same parameter order and the same default init under one torch seed
        self.conv_first = nn.Conv2d(in_chans, embed_dim, 3, 1, 1)
        self.patch_embed = _PatchEmbed(embed_dim, patch_norm)
        self.layers = nn.ModuleList([_RSTB(embed_dim, res, self.depths[i], self.num_heads[i], window_size, mlp_ratio, qkv_bias,
                                           resi_connection) for i in range(len(self.depths))])
        self.norm = nn.LayerNorm(embed_dim)
        self.conv_after_body = _resi_conv(embed_dim, resi_connection)
        if upsampler == "pixelshuffle":
            self._pixelshuffle_head(embed_dim, in_chans, upscale, num_feat)
        elif upsampler == "pixelshuffledirect":
            self.upsample = nn.Sequential(nn.Conv2d(embed_dim, upscale ** 2 * in_chans, 3, 1, 1), nn.PixelShuffle(upscale))
        elif upsampler == "nearest+conv":
            self.conv_before_upsample = conv_before_upsample(embed_dim, num_feat)
            self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            if upscale == 4:
                self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
            self.conv_last = nn.Conv2d(num_feat, in_chans, 3, 1, 1)
            self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        else:
            self.conv_last = nn.Conv2d(embed_dim, in_chans, 3, 1, 1)
        self.apply(_init_weights)
        self._init_engine_state()

    def _head_refusal(self, i: int, h: int, embed_dim: int):
        refusal = super()._head_refusal(i, h, embed_dim)
        return refusal and refusal + " (head dim)"

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

    def _make_engine(self):
        return SwinIREngine(self.img_size, self.patch_size, self.in_chans, self.embed_dim, self.depths, self.num_heads, self.window_size,
                            self.mlp_ratio, self.qkv_bias, self.qk_scale, self.ape, self.patch_norm, self.upscale, self.img_range,
                            self.upsampler, self.resi_connection)

    def forward(self, x):
        self._check_input(x, self.in_chans)
        Ho, Wo = self.out_size(int(x.shape[2]), int(x.shape[3]))
        return self._forward_only(x, self.in_chans, Ho, Wo)
