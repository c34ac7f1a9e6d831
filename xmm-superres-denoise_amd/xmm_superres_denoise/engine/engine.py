"""Thin host wrapper over the C ABI: torch supplies device memory and the HIP stream, nothing else."""
from __future__ import annotations

import ctypes
import functools

import torch

from . import _lib
from ._lib import XsdConfig, XsdError, check

STRETCH = {"linear": 0, "sqrt": 1, "asinh": 2, "log": 3}


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_cuda_f32(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise XsdError(f"{name} must be a CUDA(HIP) tensor: the MI355X engine has no CPU fallback (got {t.device})")
    if t.dtype != torch.float32:
        raise XsdError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise XsdError(f"{name} must be contiguous")


def _on_engine_device(fn):
    @functools.wraps(fn)
    def guarded(self, *a, **k):
        with torch.cuda.device(self.device_index):
            return fn(self, *a, **k)
    return guarded


def _on_tensor_device(fn):
    """the stateless entry points launch on the current stream of their first tensor's device: make that device current for the call"""
    @functools.wraps(fn)
    def guarded(t, *a, **k):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            with torch.cuda.device(t.device):
                return fn(t, *a, **k)
        return fn(t, *a, **k)       # (the argument checks of fn say what is wrong with it)
    return guarded


class Engine:
    """One engine per model instance per GPU (xsd_create / xsd_destroy)."""

    def __init__(self, kind: str, in_channels: int, out_channels: int, num_filters: int, num_res_blocks: int,
                 num_upsample: int = 1, memory_efficient: bool = False):
        self.L = _lib.load()
        cfg = XsdConfig(kind={"dn": 0, "sr": 1}[kind], in_channels=in_channels, out_channels=out_channels,
                        num_filters=num_filters, num_res_blocks=num_res_blocks, num_upsample=num_upsample,
                        memory_efficient=int(memory_efficient), reserved=0)
        h = ctypes.c_void_p()
        check(self.L.xsd_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        # The C engine allocates and launches on the CURRENT device (it never switches devices itself): every call below runs under a
        # guard for the device the engine was created on, so a process that holds modules on several GPUs, or whose current device is
        # not the module's, still puts workspace and kernels where the tensors are (one process per GPU -- the normal case -- pays a no-op)
        self.device_index = torch.cuda.current_device()
        self.kind = kind
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.scale = 2 ** num_upsample if kind == "sr" else 1
        self.nparams = int(self.L.xsd_param_count(self.h))
        self.num_stages = int(self.L.xsd_backward_num_stages(self.h))
        # The engine keeps ONE set of saved activations (one plan / workspace).  Every forward that saves them gets a new
        # generation id; a backward must name the generation it belongs to (autograd contexts do) and is refused when a
        # later forward has replaced the activations or when dy does not have the saved output's shape.
        self.generation = 0
        self._saved_gen = None
        self._saved_out_shape = None
        self._x_ref = None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.xsd_destroy(self.h)
                self.h = None
        except Exception:
            pass

    MATH = {"fp32": 0, "bf16x6": 3, "f16x3": 4}

    @_on_engine_device
    def set_math(self, mode: str):
        """'fp32' (exact fp32 MFMA), 'bf16x6' (strict: exact 3-term bf16 split, 6 products, single-rounding MFMA accumulation)
        or 'f16x3' (default: 2-term fp16 split of power-of-two-scaled operands, 22-23 significant bits per operand, 3
        products); fp32 planes in all three.  include/xsd.h: xsd_set_math."""
        if mode not in self.MATH:
            raise XsdError(f"unknown math mode {mode!r}: the modes are {sorted(self.MATH)}")
        check(self.L.xsd_set_math(self.h, self.MATH[mode]))

    def get_math(self) -> str:
        return {v: k for k, v in self.MATH.items()}[int(self.L.xsd_get_math(self.h))]

    # ---- weights
    @_on_engine_device
    def pack(self, flat_params: torch.Tensor):
        _require_cuda_f32(flat_params, "flat_params")
        if flat_params.numel() != self.nparams:
            raise XsdError(f"flat_params has {flat_params.numel()} elements, engine expects {self.nparams}")
        self._params_ref = flat_params  # keep alive: the engine reads biases from it
        check(self.L.xsd_pack_weights(self.h, flat_params.data_ptr(), _stream_ptr(flat_params.device)))

    # ---- forward / backward
    @_on_engine_device
    def forward(self, x: torch.Tensor, save_for_backward: bool = False) -> torch.Tensor:
        _require_cuda_f32(x, "x")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise XsdError(f"x must be [B,{self.in_channels},H,W] (got {tuple(x.shape)})")
        B, _, H, W = x.shape
        y = torch.empty((B, self.out_channels, H * self.scale, W * self.scale), device=x.device, dtype=torch.float32)
        check(self.L.xsd_forward(self.h, x.data_ptr(), y.data_ptr(), B, H, W, int(save_for_backward), _stream_ptr(x.device)))
        # any forward rebuilds / reuses the workspace, so previously saved activations are gone either way
        self._x_ref = x if save_for_backward else None  # conv_first's weight gradient re-reads x
        self._saved_out_shape = tuple(y.shape) if save_for_backward else None
        if save_for_backward:
            self.generation += 1
            self._saved_gen = self.generation
        else:
            self._saved_gen = None
        return y

    def has_saved(self, generation: int) -> bool:
        """True while the activations saved by forward number `generation` are still the engine's current ones."""
        return generation is not None and self._saved_gen == generation

    def _check_backward_args(self, dy, flat_grads, dx, generation):
        _require_cuda_f32(dy, "dy")
        _require_cuda_f32(flat_grads, "flat_grads")
        if self._saved_gen is None:
            raise XsdError("backward needs a preceding forward(save_for_backward=True) whose activations are still held")
        if generation is not None and generation != self._saved_gen:
            raise XsdError(f"backward for forward #{generation}, but the engine holds the activations of forward "
                           f"#{self._saved_gen}: a later forward replaced them (one saved activation set per engine)")
        if tuple(dy.shape) != self._saved_out_shape:
            raise XsdError(f"dy has shape {tuple(dy.shape)}, the saved forward produced {self._saved_out_shape}")
        if flat_grads.numel() != self.nparams:
            raise XsdError(f"flat_grads has {flat_grads.numel()} elements, engine expects {self.nparams}")
        if dx is not None:
            _require_cuda_f32(dx, "dx")
            if tuple(dx.shape) != tuple(self._x_ref.shape):
                raise XsdError(f"dx has shape {tuple(dx.shape)}, the saved input has {tuple(self._x_ref.shape)}")

    @_on_engine_device
    def backward(self, dy: torch.Tensor, flat_grads: torch.Tensor, need_dx: bool = False, generation: int | None = None):
        self._check_backward_args(dy, flat_grads, None, generation)
        dx = torch.empty_like(self._x_ref) if need_dx else None
        check(self.L.xsd_backward(self.h, dy.data_ptr(), dx.data_ptr() if need_dx else None, flat_grads.data_ptr(),
                                  _stream_ptr(dy.device)))
        return dx

    @_on_engine_device
    def backward_stage(self, stage: int, dy: torch.Tensor, flat_grads: torch.Tensor, dx: torch.Tensor | None = None,
                       generation: int | None = None):
        self._check_backward_args(dy, flat_grads, dx, generation)
        check(self.L.xsd_backward_stage(self.h, stage, dy.data_ptr(), dx.data_ptr() if dx is not None else None,
                                        flat_grads.data_ptr(), _stream_ptr(dy.device)))

    def grad_range(self, stage: int):
        off, cnt = ctypes.c_int64(), ctypes.c_int64()
        self.L.xsd_grad_range(self.h, stage, 0, ctypes.byref(off), ctypes.byref(cnt))
        return off.value, cnt.value

    # ---- loss / optimizer
    @_on_engine_device
    def l1_loss(self, y: torch.Tensor, target: torch.Tensor, want_grad: bool = True):
        _require_cuda_f32(y, "y")
        _require_cuda_f32(target, "target")
        if y.shape != target.shape:
            raise XsdError(f"shape mismatch {tuple(y.shape)} vs {tuple(target.shape)}")
        dy = torch.empty_like(y) if want_grad else None
        loss = torch.empty((), device=y.device, dtype=torch.float32)
        check(self.L.xsd_l1_loss(self.h, y.data_ptr(), target.data_ptr(), dy.data_ptr() if want_grad else None,
                                 loss.data_ptr(), y.numel(), _stream_ptr(y.device)))
        return loss, dy

    @_on_engine_device
    def adam_step(self, params, grads, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
        for n, t in (("params", params), ("grads", grads), ("m", m), ("v", v)):
            _require_cuda_f32(t, n)
        check(self.L.xsd_adam_step(self.h, params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                                   params.numel(), int(step), lr, betas[0], betas[1], eps, grad_scale,
                                   _stream_ptr(params.device)))

    # ---- measurement
    @_on_engine_device
    def profile_enable(self, on: bool):
        check(self.L.xsd_profile_enable(self.h, int(on)))

    @_on_engine_device
    def profile_read(self, klass: int):
        ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        check(self.L.xsd_profile_read(self.h, klass, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by)))
        return {"ms": ms.value, "launches": n.value, "flop": fl.value, "bytes": by.value}

    @_on_engine_device
    def probe_mfma_stream(self, fmt: str = "f16", seconds: float = 2.0):
        """dense 16-bit MFMA TFLOP/s and in-kernel clock the current device sustains on the conv's bare MFMA-wave stream
        (include/xsd.h: xsd_probe_mfma_stream); blocks for about `seconds`"""
        tf, gz = ctypes.c_double(), ctypes.c_double()
        check(self.L.xsd_probe_mfma_stream({"f16": 0, "bf16": 1}[fmt], float(seconds), ctypes.byref(tf), ctypes.byref(gz),
                                           _stream_ptr(torch.device("cuda", torch.cuda.current_device()))))
        return {"mfma_tflops": tf.value, "sclk_ghz": gz.value, "seconds": float(seconds), "fmt": fmt}


class _ForwardEngine:
    """What the forward-only engines share.  A subclass names its C functions (PREFIX + create / destroy / param_count / pack_weights /
    forward) and, in _create, its input channels, output channels and the factor between input and output size."""

    PREFIX = ""

    def __init__(self):
        self.L = _lib.load()

    def _c(self, name: str):
        return getattr(self.L, self.PREFIX + name)

    def _create(self, cfg, cin: int, cout: int, scale: int):
        h = ctypes.c_void_p()
        check(self._c("create")(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.device_index = torch.cuda.current_device()     # the C side allocates and launches on the current device (see Engine)
        self._cin, self._cout, self._scale = int(cin), int(cout), int(scale)
        self.nparams = int(self._c("param_count")(self.h))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._c("destroy")(self.h)
                self.h = None
        except Exception:
            pass

    @_on_engine_device
    def pack(self, flat_params: torch.Tensor):
        _require_cuda_f32(flat_params, "flat_params")
        if flat_params.numel() != self.nparams:
            raise XsdError(f"flat_params has {flat_params.numel()} elements, engine expects {self.nparams}")
        self._params_ref = flat_params  # keep alive: the engine reads from it whatever it does not pack (norms, biases, bias tables, ...)
        check(self._c("pack_weights")(self.h, flat_params.data_ptr(), _stream_ptr(flat_params.device)))

    @_on_engine_device
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _require_cuda_f32(x, "x")
        if x.dim() != 4 or x.shape[1] != self._cin:
            raise XsdError(f"x must be [B,{self._cin},H,W] (got {tuple(x.shape)})")
        B, _, H, W = x.shape
        Ho, Wo = self.out_size(H, W)
        y = torch.empty((B, self._cout, Ho, Wo), device=x.device, dtype=torch.float32)
        check(self._c("forward")(self.h, x.data_ptr(), y.data_ptr(), B, H, W, _stream_ptr(x.device)))
        return y

    def out_size(self, H: int, W: int) -> tuple[int, int]:
        """(Ho, Wo) of forward's output for an H x W input"""
        return H * self._scale, W * self._scale

    # ---- math mode of the GEMMs (include/xsd.h: xsd_swinfir_set_math / xsd_hat_set_math); the mode numbers of Engine.MATH
    MATH = {"fp32": 0, "bf16x6": 3}
    NAME = ""

    def set_math(self, mode: str):
        """'fp32' (default: exact fp32 MFMA) or 'bf16x6' (strict: exact 3-term bf16 split of both operands, 6 products, fp32
        accumulation) for the linear layers and the 3x3 convs; attention, LayerNorm, FFT and channel attention stay exact fp32.
        Takes effect at the next forward; no repack is needed."""
        if mode == "f16x3":
            raise XsdError(f"{self.NAME}: math mode 'f16x3' is not supported: its fp16 terms need a per-tensor scale that these kernels do "
                           f"not publish; the modes are {sorted(self.MATH)}")
        if mode not in self.MATH:
            raise XsdError(f"{self.NAME}: unknown math mode {mode!r}: the modes are {sorted(self.MATH)}")
        check(self._c("set_math")(self.h, self.MATH[mode]))

    def get_math(self) -> str:
        return {v: k for k, v in self.MATH.items()}[int(self._c("get_math")(self.h))]


class RestormerEngine(_ForwardEngine):
    """One Restormer engine per module per GPU (xsd_restormer_create / _destroy): forward only."""

    PREFIX = "xsd_restormer_"
    NAME = "Restormer"
    MATH = {"fp32": 0}

    def set_math(self, mode: str):
        """Restormer's kernels are exact fp32 on the vector ALUs: 'fp32' is the only mode."""
        if mode != "fp32":
            raise XsdError(f"Restormer: math mode {mode!r} is not supported: the Restormer engine computes in 'fp32' only")

    def get_math(self) -> str:
        return "fp32"

    def __init__(self, inp_channels: int, out_channels: int, dim: int, num_blocks, num_refinement_blocks: int, heads,
                 ffn_expansion_factor: float, bias: bool, layernorm_bias_free: bool):
        super().__init__()
        cfg = _lib.XsdRestormerConfig(inp_channels=inp_channels, out_channels=out_channels, dim=dim,
                                      num_blocks=(ctypes.c_int32 * 4)(*num_blocks), num_refinement_blocks=num_refinement_blocks,
                                      heads=(ctypes.c_int32 * 4)(*heads), bias=int(bias), layernorm_bias_free=int(layernorm_bias_free),
                                      dual_pixel_task=0, ffn_expansion_factor=float(ffn_expansion_factor))
        self._create(cfg, inp_channels, out_channels, 1)
        self.in_channels, self.out_channels = int(inp_channels), int(out_channels)


class _SwinEngine(_ForwardEngine):
    """What the SwinFIR, HAT and SwinIR engines share: the 17 configuration fields their C structs have in common.  A subclass names its
    struct (CONFIG), its resi_connection forms (RESI; an unknown one gets the index behind the last, which create refuses) and, in
    `extra`, the fields of its own."""

    UPSAMPLERS = ("pixelshuffle", "pixelshuffledirect", "nearest+conv", "")
    CONFIG = None
    RESI = ()

    def _upsampler_index(self, upsampler: str) -> int:
        return self.UPSAMPLERS.index(upsampler) if upsampler in self.UPSAMPLERS else 3

    def __init__(self, img_size, patch_size, in_chans: int, embed_dim: int, depths, num_heads, window_size: int, mlp_ratio: float,
                 qkv_bias: bool, qk_scale, ape: bool, patch_norm: bool, upscale: int, img_range: float, upsampler: str,
                 resi_connection: str, **extra):
        super().__init__()
        depths, num_heads = [int(d) for d in depths], [int(h) for h in num_heads]
        if len(depths) > 16 or len(num_heads) < len(depths):
            raise XsdError(f"{self.NAME}: at most 16 layers with one num_heads entry each (got depths {depths}, num_heads {num_heads})")
        cfg = self.CONFIG(img_size=(ctypes.c_int32 * 2)(*img_size), patch_size=(ctypes.c_int32 * 2)(*patch_size),
                          in_chans=int(in_chans), embed_dim=int(embed_dim), num_layers=len(depths),
                          depths=(ctypes.c_int32 * 16)(*depths), num_heads=(ctypes.c_int32 * 16)(*num_heads[:len(depths)]),
                          window_size=int(window_size), qkv_bias=int(bool(qkv_bias)), ape=int(bool(ape)),
                          patch_norm=int(bool(patch_norm)), upscale=int(upscale),
                          upsampler=self._upsampler_index(upsampler),
                          resi_connection=self.RESI.index(resi_connection) if resi_connection in self.RESI else len(self.RESI),
                          mlp_ratio=float(mlp_ratio), qk_scale=float(qk_scale or 0.0), img_range=float(img_range), **extra)
        self._create(cfg, in_chans, in_chans, upscale)
        self.in_chans, self.upscale = int(in_chans), int(upscale)


class SwinFIREngine(_SwinEngine):
    """One SwinFIR engine per module per GPU (xsd_swinfir_create / _destroy): forward only."""

    CONFIG = _lib.XsdSwinFIRConfig
    RESI = ("SFB", "1conv", "HSFB", "identity")
    PREFIX = "xsd_swinfir_"
    NAME = "SwinFIR"

    @_on_engine_device
    def fourier_pair(self, x: torch.Tensor, spec: torch.Tensor | None = None) -> torch.Tensor:
        """The FourierUnit's transforms on their own (tests): x [B,H,W,C2] fp32 -> spectrum [B,H,W//2+1,C2,2] = rfftn(x, dim=(1,2),
        norm="ortho"); given `spec`, returns x + irfftn(spec, s=(H,W), dim=(1,2), norm="ortho") instead (spec is overwritten)."""
        _require_cuda_f32(x, "x")
        B, H, W, C2 = x.shape
        x = x.contiguous().clone()
        if spec is None:
            out = torch.empty((B, H, W // 2 + 1, C2, 2), device=x.device, dtype=torch.float32)
            check(self.L.xsd_swinfir_test_fft(self.h, x.data_ptr(), out.data_ptr(), B, H, W, C2, 0, _stream_ptr(x.device)))
            return out
        _require_cuda_f32(spec, "spec")
        spec = spec.contiguous().clone()
        check(self.L.xsd_swinfir_test_fft(self.h, x.data_ptr(), spec.data_ptr(), B, H, W, C2, 1, _stream_ptr(x.device)))
        return x


class HATEngine(_SwinEngine):
    """One HAT engine per module per GPU (xsd_hat_create / _destroy): forward only."""

    CONFIG = _lib.XsdHATConfig
    RESI = ("1conv", "identity")
    PREFIX = "xsd_hat_"
    NAME = "HAT"

    def __init__(self, img_size, patch_size, in_chans: int, embed_dim: int, depths, num_heads, window_size: int, compress_ratio: int,
                 squeeze_factor: int, conv_scale: float, overlap_ratio: float, mlp_ratio: float, qkv_bias: bool, qk_scale, ape: bool,
                 patch_norm: bool, upscale: int, img_range: float, upsampler: str, resi_connection: str):
        super().__init__(img_size, patch_size, in_chans, embed_dim, depths, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale, ape,
                         patch_norm, upscale, img_range, upsampler, resi_connection, compress_ratio=int(compress_ratio),
                         squeeze_factor=int(squeeze_factor), conv_scale=float(conv_scale), overlap_ratio=float(overlap_ratio))


class SwinIREngine(_SwinEngine):
    """One SwinIR engine per module per GPU (xsd_swinir_create / _destroy): forward only, any image size (the engine reflect-pads to
    multiples of window_size and crops back)."""

    CONFIG = _lib.XsdSwinIRConfig
    RESI = ("1conv", "3conv")
    PREFIX = "xsd_swinir_"
    NAME = "SwinIR"

    def _upsampler_index(self, upsampler: str) -> int:
        if upsampler not in self.UPSAMPLERS:       # "" is a head of SwinIR's: an unknown name must not become it
            raise XsdError(f"SwinIR: unknown upsampler {upsampler!r}: {self.UPSAMPLERS}")
        return self.UPSAMPLERS.index(upsampler)

    def out_size(self, H: int, W: int) -> tuple[int, int]:
        """(Ho, Wo) of forward's output for an H x W input (xsd_swinir_out_size): H upscale x W upscale for every head that enlarges;
        raises XsdError for the sizes the forward refuses.  Host arithmetic: no device work."""
        ho, wo = ctypes.c_int(), ctypes.c_int()
        check(self.L.xsd_swinir_out_size(self.h, int(H), int(W), ctypes.byref(ho), ctypes.byref(wo)))
        return ho.value, wo.value


@_on_tensor_device
def swinir_pad(x: torch.Tensor, ws: int, mean=None, img_range: float = 1.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """check_image_size and the input affine of SwinIR on their own (include/xsd.h: xsd_swinir_test_pad): x [B, C, H, W] ->
    (F.pad(x, (0, pw, 0, ph), "reflect") - mean) * img_range with H + ph and W + pw the next multiples of ws; mean: C numbers or None."""
    _require_cuda_f32(x, "x")
    if x.dim() != 4:
        raise XsdError(f"x {tuple(x.shape)} is not [B, C, H, W]")
    B, C, H, W = (int(v) for v in x.shape)
    ws = int(ws)
    if ws < 1:
        raise XsdError(f"window size {ws} must be positive")
    shape = (B, C, H + (ws - H % ws) % ws, W + (ws - W % ws) % ws)
    out = _out_like(out, shape, x.device, "out")
    m = None
    if mean is not None:
        mean = [float(v) for v in mean]
        if len(mean) != C:
            raise XsdError(f"mean has {len(mean)} entries for {C} channels")
        m = (ctypes.c_float * C)(*mean)
    check(_lib.load().xsd_swinir_test_pad(x.data_ptr(), out.data_ptr(), B, C, H, W, ws, m, float(img_range), _stream_ptr(x.device)))
    return out


@_on_tensor_device
def swinir_nearest_conv(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, slope: float = 0.2, math: str = "fp32",
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """lrelu(conv3x3(nearest2x(a))) of SwinIR's "nearest+conv" head on its own (include/xsd.h: xsd_swinir_test_nearest_conv): a [B, H, W, cin]
    token-major, w [N, cin, 3, 3] -> [B, 2 H, 2 W, N] token-major; the upsampled image is never stored."""
    _require_cuda_f32(a, "a")
    _require_cuda_f32(w, "w")
    if a.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (a.shape[3], 3, 3):
        raise XsdError(f"a {tuple(a.shape)} and w {tuple(w.shape)} are not [B, H, W, cin] and [N, cin, 3, 3]")
    if math not in SW_MATH:
        raise XsdError(f"unknown math mode {math!r}: the modes are {sorted(SW_MATH)}")
    B, H, W, cin = (int(v) for v in a.shape)
    N = int(w.shape[0])
    if bias is not None:
        _require_cuda_f32(bias, "bias")
        if bias.numel() != N:
            raise XsdError(f"bias has {bias.numel()} elements for {N} outputs")
    out = _out_like(out, (B, 2 * H, 2 * W, N), a.device, "out")
    check(_lib.load().xsd_swinir_test_nearest_conv(a.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, H, W, cin, N, float(slope),
                                                   SW_MATH[math], _stream_ptr(a.device)))
    return out


@_on_tensor_device
def hat_ocab_attention(qkv: torch.Tensor, table: torch.Tensor, H: int, W: int, heads: int, ws: int, ow: int, scale: float) -> torch.Tensor:
    """The OCAB's attention on its own (include/xsd.h: xsd_hat_test_ocab): qkv [B, H W, 3 C] token rows (the qkv Linear's output), table
    [(ws + ow - 1)^2, heads] -> [B, H W, C], the input of proj."""
    _require_cuda_f32(qkv, "qkv")
    _require_cuda_f32(table, "table")
    B, L, C3 = qkv.shape
    if L != H * W or C3 % 3 or tuple(table.shape) != ((ws + ow - 1) ** 2, heads):
        raise XsdError(f"qkv {tuple(qkv.shape)} / table {tuple(table.shape)} do not fit {H} x {W}, {heads} heads, windows {ws} / {ow}")
    out = torch.empty((B, L, C3 // 3), device=qkv.device, dtype=torch.float32)
    check(_lib.load().xsd_hat_test_ocab(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, C3 // 3, heads, ws, ow, float(scale),
                                        _stream_ptr(qkv.device)))
    return out


SW_ACT = {None: 0, "gelu": 1, "lrelu": 2}
SW_MATH = {"fp32": 0, "bf16x6": 3}


def _sw_test_gemm(a, w, bias, act, math, conv3, B, H, W, cin, out):
    _require_cuda_f32(a, "a")
    _require_cuda_f32(w, "w")
    if act not in SW_ACT:
        raise XsdError(f"unknown activation {act!r}: {list(SW_ACT)}")
    if math not in SW_MATH:
        raise XsdError(f"unknown math mode {math!r}: the modes are {sorted(SW_MATH)}")
    N = int(w.shape[0])
    if bias is not None:
        _require_cuda_f32(bias, "bias")
        if bias.numel() != N:
            raise XsdError(f"bias has {bias.numel()} elements for {N} outputs")
    rows = B * H * W
    if out is None:
        out = torch.empty((rows, N), device=a.device, dtype=torch.float32)
    else:
        _require_cuda_f32(out, "out")
        if out.dim() != 2 or out.shape[0] < rows or out.shape[1] < N:
            raise XsdError(f"out {tuple(out.shape)} does not hold {rows} x {N}")
    check(_lib.load().xsd_sw_test_gemm(a.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                       int(conv3), B, H, W, cin, N, int(out.shape[1]), SW_ACT[act], 0.01, SW_MATH[math],
                                       _stream_ptr(a.device)))
    return out


@_on_tensor_device
def sw_gemm(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None, math: str = "fp32",
            out: torch.Tensor | None = None) -> torch.Tensor:
    """The GEMM of the SwinFIR / HAT engines on its own (include/xsd.h: xsd_sw_test_gemm): a [M, K] token rows, w [N, K] as a Linear
    stores it -> act(a w^T + bias) [M, N]; act None, "gelu" (exact erf) or "lrelu" (slope 0.01); math "fp32" or "bf16x6".  With `out`
    (2-D, at least M x N, contiguous) the result goes into its first M rows and N columns and nothing else of it is written."""
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[1]:
        raise XsdError(f"a {tuple(a.shape)} and w {tuple(w.shape)} are not [M, K] and [N, K]")
    return _sw_test_gemm(a, w, bias, act, math, False, 1, 1, int(a.shape[0]), int(a.shape[1]), out)


@_on_tensor_device
def sw_conv3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, math: str = "fp32", act: str | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """The same GEMM as the implicit im2col of a 3x3 conv (zero padding 1): x [B, H, W, cin] token-major, w [N, cin, 3, 3] as a Conv2d
    stores it -> [B, H, W, N] token-major (with `out`: as sw_gemm, rows = B H W)."""
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (x.shape[3], 3, 3):
        raise XsdError(f"x {tuple(x.shape)} and w {tuple(w.shape)} are not [B, H, W, cin] and [N, cin, 3, 3]")
    B, H, W, cin = (int(v) for v in x.shape)
    y = _sw_test_gemm(x, w, bias, act, math, True, B, H, W, cin, out)
    return y if out is not None else y.view(B, H, W, -1)


SW_OMODE = {"tok": 0, "shuffle": 1, "nchw": 2, "shuffle_nchw": 3}


@_on_tensor_device
def sw_gemm_view(a: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, conv3: bool, B: int, H: int, W: int, cin: int, N: int,
                 ext: bool = False, a_nchw: bool = False, lda: int = 0, imean: torch.Tensor | None = None, irange: float = 1.0,
                 bias: torch.Tensor | None = None, act: str | None = None, slope: float = 0.0, res: torch.Tensor | None = None,
                 rbs: int = 0, rps: int = 0, omode: str = "tok", ldy: int = 0, r: int = 1, omean: torch.Tensor | None = None,
                 orange: float = 1.0, math: str = "fp32", rnchw: bool = False, cH: int = 0, cW: int = 0, up2: bool = False) -> torch.Tensor:
    """One launch of the Swin GEMM described as the forwards describe theirs (include/xsd.h: xsd_sw_gemm_view), on the instance SwinFIR
    runs or, with `ext`, on SwinIR's.  Tensors stand for device addresses only: the kernel reads and writes from each tensor's first
    element with the strides given here, so a view that starts inside a larger buffer (a column slice, a shifted base) is passed as
    that view.  The caller sizes the buffers.  Returns y."""
    for name, t in (("a", a), ("w", w), ("y", y), ("bias", bias), ("res", res), ("imean", imean), ("omean", omean)):
        if t is None:
            if name in ("a", "w", "y"):
                raise XsdError(f"{name} is missing")
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise XsdError(f"{name} must be a float32 CUDA(HIP) tensor")
    if act not in SW_ACT:
        raise XsdError(f"unknown activation {act!r}: {list(SW_ACT)}")
    if math not in SW_MATH:
        raise XsdError(f"unknown math mode {math!r}: the modes are {sorted(SW_MATH)}")
    if omode not in SW_OMODE:
        raise XsdError(f"unknown omode {omode!r}: {list(SW_OMODE)}")
    if w.numel() != N * cin * (9 if conv3 else 1) or not w.is_contiguous():
        raise XsdError(f"w {tuple(w.shape)} is not the contiguous [N = {N}, cin = {cin}{', 3, 3' if conv3 else ''}] weight")
    if bias is not None and bias.numel() != N:
        raise XsdError(f"bias has {bias.numel()} elements for {N} outputs")
    if imean is not None and imean.numel() != cin:
        raise XsdError(f"imean has {imean.numel()} elements for {cin} input channels")
    nmean = N if omode == "nchw" else N // max(1, r * r)
    if omean is not None and omean.numel() != nmean:
        raise XsdError(f"omean has {omean.numel()} elements for {nmean} output channels")
    v = _lib.XsdSwGemmView(conv3=int(bool(conv3)), B=int(B), H=int(H), W=int(W), cin=int(cin), N=int(N), a=a.data_ptr(),
                           a_nchw=int(bool(a_nchw)), lda=int(lda), imean=_ptr(imean), irange=float(irange), w=w.data_ptr(),
                           bias=_ptr(bias), act=SW_ACT[act], slope=float(slope), res=_ptr(res), rbs=int(rbs), rps=int(rps),
                           omode=SW_OMODE[omode], y=y.data_ptr(), ldy=int(ldy), r=int(r), omean=_ptr(omean), orange=float(orange),
                           math=SW_MATH[math], rnchw=int(bool(rnchw)), cH=int(cH), cW=int(cW), up2=int(bool(up2)))
    L = _lib.load()
    check((L.xsd_swinir_test_gemm_view if ext else L.xsd_sw_test_gemm_view)(ctypes.byref(v), _stream_ptr(a.device)))
    return y


@_on_tensor_device
def hat_channel_mean(x: torch.Tensor) -> torch.Tensor:
    """The channel attention's global average pool on its own (include/xsd.h: xsd_hat_test_channel_mean): x [B, HW, C] token-major ->
    [B, C] means, summed in double in a fixed order."""
    _require_cuda_f32(x, "x")
    B, HW, C = x.shape
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    check(_lib.load().xsd_hat_test_channel_mean(x.data_ptr(), out.data_ptr(), B, HW, C, _stream_ptr(x.device)))
    return out


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _out_like(out, shape, device, what):
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    _require_cuda_f32(out, what)
    if tuple(out.shape) != tuple(shape):
        raise XsdError(f"{what} {tuple(out.shape)} is not {tuple(shape)}")
    return out


@_on_tensor_device
def sw_window_attention(qkv: torch.Tensor, table: torch.Tensor, H: int, W: int, heads: int, ws: int, shift: int, scale: float,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """The shifted-window attention of SwinFIR and HAT on its own (include/xsd.h: xsd_sw_test_attention): qkv [B, H W, 3 C] token rows in
    image order (the qkv Linear's output), table [(2 ws - 1)^2, heads] -> [B, H W, C], the input of proj, in image order (into `out` if
    given)."""
    _require_cuda_f32(qkv, "qkv")
    _require_cuda_f32(table, "table")
    B, L, C3 = qkv.shape
    if L != H * W or C3 % 3 or tuple(table.shape) != ((2 * ws - 1) ** 2, heads):
        raise XsdError(f"qkv {tuple(qkv.shape)} / table {tuple(table.shape)} do not fit {H} x {W}, {heads} heads, window {ws}")
    out = _out_like(out, (B, L, C3 // 3), qkv.device, "out")
    check(_lib.load().xsd_sw_test_attention(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, C3 // 3, heads, ws, shift, float(scale),
                                            _stream_ptr(qkv.device)))
    return out


@_on_tensor_device
def sw_layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The token LayerNorm of SwinFIR and HAT on its own (include/xsd.h: xsd_sw_test_layernorm): x [M, C], w and b [C] -> [M, C].  With
    `out` (2-D, C columns, at least M rows, contiguous) the result goes into its first M rows and nothing else of it is written."""
    _require_cuda_f32(x, "x")
    _require_cuda_f32(w, "w")
    _require_cuda_f32(b, "b")
    if x.dim() != 2 or w.numel() != x.shape[1] or b.numel() != x.shape[1]:
        raise XsdError(f"x {tuple(x.shape)}, w {tuple(w.shape)} and b {tuple(b.shape)} are not [M, C], [C] and [C]")
    M, C = (int(v) for v in x.shape)
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=torch.float32)
    else:
        _require_cuda_f32(out, "out")
        if out.dim() != 2 or out.shape[0] < M or out.shape[1] != C:
            raise XsdError(f"out {tuple(out.shape)} does not hold {M} rows of {C}")
    check(_lib.load().xsd_sw_test_layernorm(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), M, C, _stream_ptr(x.device)))
    return out


@_on_tensor_device
def hat_ca_combine(x: torch.Tensor, t: torch.Tensor, w1: torch.Tensor | None = None, b1: torch.Tensor | None = None,
                   w2: torch.Tensor | None = None, b2: torch.Tensor | None = None, scale: float = 1.0,
                   gates: torch.Tensor | None = None) -> torch.Tensor:
    """What a HAB does with its CAB branch, on its own (include/xsd.h: xsd_hat_test_ca_combine): x, t [B, HW, C] token-major, w1 [Cs, C],
    b1 [Cs], w2 [C, Cs], b2 [C] -> x += t * sigmoid(w2 relu(w1 mean(t) + b1) + b2) * scale IN PLACE (x is returned); `gates` [B, C]
    receives the sigmoid gates.  Without w1: the plain x += t * scale."""
    _require_cuda_f32(x, "x")
    _require_cuda_f32(t, "t")
    if x.dim() != 3 or x.shape != t.shape:
        raise XsdError(f"x {tuple(x.shape)} and t {tuple(t.shape)} are not the same [B, HW, C]")
    B, HW, C = (int(v) for v in x.shape)
    Cs = 0
    if w1 is not None:
        for n, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
            _require_cuda_f32(v, n)
        Cs = int(b1.numel())
        if w1.numel() != Cs * C or w2.numel() != C * Cs or b2.numel() != C:
            raise XsdError(f"w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, w2 {tuple(w2.shape)}, b2 {tuple(b2.shape)} are not a squeeze MLP of {C} channels")
    if gates is not None:
        _out_like(gates, (B, C), x.device, "gates")
    check(_lib.load().xsd_hat_test_ca_combine(x.data_ptr(), t.data_ptr(), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), float(scale), B, HW, C, Cs,
                                              _ptr(gates), _stream_ptr(x.device)))
    return x


RST_LN = {None: 0, "WithBias": 1, "BiasFree": 2}


@_on_tensor_device
def restormer_pw(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, ln: str | None = None,
                 ln_weight: torch.Tensor | None = None, ln_bias: torch.Tensor | None = None, residual: bool = False,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Restormer's 1x1 conv on its own (include/xsd.h: xsd_restormer_test_pw): x [B, Cx, HW] of which the first cin channels are read,
    w [cout, cin] as a Conv2d stores it or [B, cout, cin] (one matrix per image); ln None, "WithBias" or "BiasFree" (the channel LayerNorm
    in front).  The result goes to the first cout channels of `out` [B, Cy, HW] (nothing else of it is written); with `residual` it is
    added to them in place."""
    _require_cuda_f32(x, "x")
    _require_cuda_f32(w, "w")
    if ln not in RST_LN:
        raise XsdError(f"unknown LayerNorm type {ln!r}: {list(RST_LN)}")
    if x.dim() != 3 or w.dim() not in (2, 3) or (w.dim() == 3 and w.shape[0] != x.shape[0]) or w.shape[-1] > x.shape[1]:
        raise XsdError(f"x {tuple(x.shape)} and w {tuple(w.shape)} are not [B, >= cin, HW] and [(B,) cout, cin]")
    B, Cx, HW = (int(v) for v in x.shape)
    cout, cin = int(w.shape[-2]), int(w.shape[-1])
    for n, v, k in (("bias", bias, cout), ("ln_weight", ln_weight, cin), ("ln_bias", ln_bias, cin)):
        if v is not None:
            _require_cuda_f32(v, n)
            if v.numel() != k:
                raise XsdError(f"{n} has {v.numel()} elements, not {k}")
    if out is None:
        if residual:
            raise XsdError("residual needs the `out` it adds to")
        out = torch.empty((B, cout, HW), device=x.device, dtype=torch.float32)
    else:
        _require_cuda_f32(out, "out")
        if out.dim() != 3 or out.shape[0] != B or out.shape[1] < cout or out.shape[2] != HW:
            raise XsdError(f"out {tuple(out.shape)} does not hold {B} x {cout} x {HW}")
    check(_lib.load().xsd_restormer_test_pw(x.data_ptr(), Cx * HW, w.data_ptr(), int(w.dim() == 3), _ptr(bias), RST_LN[ln], _ptr(ln_weight),
                                            _ptr(ln_bias), int(bool(residual)), out.data_ptr(), int(out.shape[1]) * HW, B, cin, cout, HW,
                                            _stream_ptr(x.device)))
    return out


@_on_tensor_device
def restormer_dw(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, gate: bool = False,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Restormer's depthwise 3x3 conv on its own (include/xsd.h: xsd_restormer_test_dw): x [B, Cin, H, W], w [Cin, 1, 3, 3] -> [B, Cin, H, W];
    with `gate`, gelu(x1) * x2 of the conv's two channel halves -> [B, Cin / 2, H, W]."""
    _require_cuda_f32(x, "x")
    _require_cuda_f32(w, "w")
    if x.dim() != 4 or w.numel() != 9 * x.shape[1] or (gate and x.shape[1] % 2):
        raise XsdError(f"x {tuple(x.shape)} and w {tuple(w.shape)} are not [B, Cin, H, W] and [Cin, 1, 3, 3]")
    B, Cin, H, W = (int(v) for v in x.shape)
    if bias is not None:
        _require_cuda_f32(bias, "bias")
        if bias.numel() != Cin:
            raise XsdError(f"bias has {bias.numel()} elements, not {Cin}")
    cout = Cin // 2 if gate else Cin
    out = _out_like(out, (B, cout, H, W), x.device, "out")
    check(_lib.load().xsd_restormer_test_dw(x.data_ptr(), w.data_ptr(), _ptr(bias), out.data_ptr(), B, cout, int(bool(gate)), H, W,
                                            _stream_ptr(x.device)))
    return out


def _restormer_attention(entry, qkv, temperature, w_po, b_po, x, heads):
    for n, v in (("qkv", qkv), ("temperature", temperature), ("w_po", w_po), ("x", x)):
        _require_cuda_f32(v, n)
    if x.dim() != 3 or tuple(qkv.shape) != (x.shape[0], 3 * x.shape[1], x.shape[2]) or w_po.numel() != x.shape[1] ** 2 or \
            temperature.numel() != heads:
        raise XsdError(f"qkv {tuple(qkv.shape)}, temperature {tuple(temperature.shape)}, w_po {tuple(w_po.shape)} and x {tuple(x.shape)} do not fit "
                       f"[B, 3 C, HW], [{heads}], [C, C] and [B, C, HW]")
    B, C, HW = (int(v) for v in x.shape)
    if b_po is not None:
        _require_cuda_f32(b_po, "b_po")
        if b_po.numel() != C:
            raise XsdError(f"b_po has {b_po.numel()} elements, not {C}")
    check(getattr(_lib.load(), entry)(qkv.data_ptr(), temperature.data_ptr(), w_po.data_ptr(), _ptr(b_po), x.data_ptr(), B, C, int(heads), HW,
                                      _stream_ptr(x.device)))
    return x


@_on_tensor_device
def restormer_channel_attention(qkv: torch.Tensor, temperature: torch.Tensor, w_po: torch.Tensor, b_po: torch.Tensor | None,
                                x: torch.Tensor, heads: int) -> torch.Tensor:
    """Restormer's channel attention behind the depthwise conv, on its own (include/xsd.h: xsd_restormer_test_attention): qkv
    [B, 3 C, HW], temperature [heads], w_po [C, C] (project_out as stored), b_po [C] or None; x [B, C, HW] is updated IN PLACE,
    x += project_out(softmax(normalize(q) normalize(k)^T temperature) v), and returned.  At most 64 channels per head."""
    return _restormer_attention("xsd_restormer_test_attention", qkv, temperature, w_po, b_po, x, heads)


@_on_tensor_device
def restormer_channel_attention_wide(qkv: torch.Tensor, temperature: torch.Tensor, w_po: torch.Tensor, b_po: torch.Tensor | None,
                                     x: torch.Tensor, heads: int) -> torch.Tensor:
    """The same through the wide kernels (include/xsd.h: xsd_restormer_test_attention_wide), which the forward runs from 65 to 128
    channels per head: here at any width up to 128, bitwise equal to restormer_channel_attention where both run."""
    return _restormer_attention("xsd_restormer_test_attention_wide", qkv, temperature, w_po, b_po, x, heads)


RST_CONV3 = {None: 0, "unshuffle": 1, "shuffle": 2}


@_on_tensor_device
def restormer_conv3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, skip: torch.Tensor | None = None,
                      mode: str | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Restormer's dense 3x3 conv on its own (include/xsd.h: xsd_restormer_test_conv3): x [B, cin, H, W], w [cout, cin, 3, 3] ->
    [B, cout, H, W] (+ skip); mode "unshuffle": PixelUnshuffle(2) of it, [B, 4 cout, H / 2, W / 2]; "shuffle": PixelShuffle(2) of it,
    [B, cout / 4, 2 H, 2 W]."""
    _require_cuda_f32(x, "x")
    _require_cuda_f32(w, "w")
    if mode not in RST_CONV3:
        raise XsdError(f"unknown mode {mode!r}: {list(RST_CONV3)}")
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (x.shape[1], 3, 3):
        raise XsdError(f"x {tuple(x.shape)} and w {tuple(w.shape)} are not [B, cin, H, W] and [cout, cin, 3, 3]")
    B, cin, H, W = (int(v) for v in x.shape)
    cout = int(w.shape[0])
    if bias is not None:
        _require_cuda_f32(bias, "bias")
        if bias.numel() != cout:
            raise XsdError(f"bias has {bias.numel()} elements, not {cout}")
    if skip is not None:
        _require_cuda_f32(skip, "skip")
        if tuple(skip.shape) != (B, cout, H, W):
            raise XsdError(f"skip {tuple(skip.shape)} is not {(B, cout, H, W)}")
    shape = (B, cout, H, W)
    if mode == "unshuffle":
        if H % 2 or W % 2:
            raise XsdError(f"PixelUnshuffle(2) of {H} x {W} has no output shape: H and W must be even")
        shape = (B, 4 * cout, H // 2, W // 2)
    elif mode == "shuffle":
        if cout % 4:
            raise XsdError(f"PixelShuffle(2) of {cout} channels has no output shape: cout must be a multiple of 4")
        shape = (B, cout // 4, 2 * H, 2 * W)
    out = _out_like(out, shape, x.device, "out")
    check(_lib.load().xsd_restormer_test_conv3(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(skip), out.data_ptr(), B, cin, cout, H, W,
                                               RST_CONV3[mode], _stream_ptr(x.device)))
    return out


def _copy_stage(call, out, device, layout):
    """shared by ExtMetricsEngine.stage and FsimEngine.stage: `call(ptr, nbytes, info)` is the C hook, which fills `info` before it
    judges the buffer; without `out` a first call with an 8-byte buffer learns the region's dims (a region that small is simply
    copied), a second one copies into a tensor of the right size.  layout(info) -> (dtype, shape)."""
    info = (ctypes.c_int32 * 8)()
    if out is None:
        probe = torch.empty(8, device=device, dtype=torch.uint8)
        rc = call(probe.data_ptr(), 8, info)
        if rc != 0 and b"buffer too small" not in _lib.load().xsd_last_error():
            check(rc)
        dtype, shape = layout(info)
        out = torch.empty(shape, device=device, dtype=dtype)
        check(call(out.data_ptr(), out.numel() * out.element_size(), info))
    else:
        if not out.is_cuda or not out.is_contiguous():
            raise XsdError("out must be a contiguous device tensor")
        check(call(out.data_ptr(), out.numel() * out.element_size(), info))
        dtype, shape = layout(info)
        if out.dtype != dtype:
            raise XsdError(f"out is {out.dtype}, the region is {dtype}")
        n = 1
        for k in shape:
            n *= k
        out = out.reshape(-1)[:n].reshape(shape)
    keys = ("B", "h", "w", "entries", "tiles_x", "ntiles", "tile_h", "tile_w")
    return out, dict(zip(keys, (int(v) for v in info)))


class ExtMetricsEngine:
    """The extended test metrics of one batch (include/xsd.h: xsd_ext_metrics_eval): gmsd, ms_gmsd, haarpsi, mdsi and the two
    VIF sums per image, as doubles.  The formulas restate piq 0.7.x / torchmetrics 1.x from their published code; parity with
    the libraries themselves is unpinned.  One object per GPU; it owns a device workspace."""

    OUT = 6          # XSD_EXTM_OUT: gmsd, ms_gmsd, haarpsi, mdsi, vif numerator, vif denominator

    def __init__(self):
        self.L = _lib.load()
        h = ctypes.c_void_p()
        check(self.L.xsd_ext_metrics_create(ctypes.byref(h)))
        self.h = h
        self.device_index = torch.cuda.current_device()     # the C side allocates and launches on the current device (see Engine)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.xsd_ext_metrics_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @_on_engine_device
    def eval(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """preds, target: [B, H, W] (or [B, 1, H, W]) fp32 in [0, 1] on this engine's device -> [B, 6] float64 per-image values"""
        _require_cuda_f32(preds, "preds")
        _require_cuda_f32(target, "target")
        if preds.shape != target.shape:
            raise XsdError(f"shape mismatch {tuple(preds.shape)} vs {tuple(target.shape)}")
        if preds.dim() == 4 and preds.shape[1] == 1:
            preds, target = preds[:, 0], target[:, 0]
        if preds.dim() != 3:
            raise XsdError(f"expected [B,H,W] or [B,1,H,W], got {tuple(preds.shape)}")
        if preds.device.index != self.device_index:
            raise XsdError(f"preds is on cuda:{preds.device.index}, this engine's workspace on cuda:{self.device_index}")
        B, H, W = preds.shape
        out = torch.empty((B, self.OUT), device=preds.device, dtype=torch.float64)
        check(self.L.xsd_ext_metrics_eval(self.h, preds.data_ptr(), target.data_ptr(), out.data_ptr(), B, H, W, _stream_ptr(preds.device)))
        return out

    # the regions xsd_ext_metrics_test_stage copies out (include/xsd.h: XSD_EXTM_STAGE_*)
    STAGES = ("u1", "u2", "u3", "m", "v1", "v2", "v3", "gms0", "gms1", "gms2", "gms3", "haar", "mdsi1", "mdsi2", "vif0", "vif1", "vif2", "vif3")

    @_on_engine_device
    def stage(self, name: str, side: int = 0, out: torch.Tensor | None = None):
        """One region of the last eval's workspace (include/xsd.h: xsd_ext_metrics_test_stage) -> (tensor, info).  An image
        ("u1".."u3", "m", "v1".."v3"; side 0 = preds, 1 = target) is fp32 [B, h, w]; tile partials ("gms0".."gms3", "haar", "mdsi1",
        "mdsi2", "vif0".."vif3") are float64 [B, ntiles, entries].  info: dict(B, h, w, entries, tiles_x, ntiles, tile_h, tile_w).  The
        copy goes into `out` (a contiguous device tensor of the region's dtype and at least its size, reshaped) if given."""
        if name not in self.STAGES:
            raise XsdError(f"unknown stage {name!r} (one of {self.STAGES})")
        return _copy_stage(lambda ptr, nbytes, info: self.L.xsd_ext_metrics_test_stage(self.h, self.STAGES.index(name), int(side), ptr, nbytes, info,
                                                                                       _stream_ptr(torch.device("cuda", self.device_index))),
                           out, torch.device("cuda", self.device_index),
                           lambda i: (torch.float64, (i[0], i[5], i[3])) if i[3] else (torch.float32, (i[0], i[1], i[2])))


class FsimEngine:
    """fsim of one batch (include/xsd.h: xsd_fsim_eval): piq 0.7.x fsim(chromatic=False) per image, as doubles.  The formula restates
    piq's published code (tests/golden/fsim_torch.py); parity with piq itself is unpinned.  One object per GPU; it
    owns a device workspace and the plans (filters, DFT matrices) of the pooled sizes it has seen most recently."""

    def __init__(self):
        self.L = _lib.load()
        h = ctypes.c_void_p()
        check(self.L.xsd_fsim_create(ctypes.byref(h)))
        self.h = h
        self.device_index = torch.cuda.current_device()     # the C side allocates and launches on the current device (see Engine)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.xsd_fsim_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _mine(self, t: torch.Tensor, name: str):
        _require_cuda_f32(t, name)
        if t.device.index != self.device_index:
            raise XsdError(f"{name} is on cuda:{t.device.index}, this engine's workspace on cuda:{self.device_index}")

    @_on_engine_device
    def eval(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """preds, target: [B, H, W] or [B, 1, H, W] fp32 in [0, 1] on this engine's device -> [B] float64 per-image fsim"""
        self._mine(preds, "preds")
        self._mine(target, "target")
        if preds.shape != target.shape:
            raise XsdError(f"shape mismatch {tuple(preds.shape)} vs {tuple(target.shape)}")
        if preds.dim() == 3:
            preds, target = preds[:, None], target[:, None]
        if preds.dim() != 4:
            raise XsdError(f"expected [B,H,W] or [B,1,H,W], got {tuple(preds.shape)}")
        B, C, H, W = preds.shape
        out = torch.empty((B,), device=preds.device, dtype=torch.float64)
        check(self.L.xsd_fsim_eval(self.h, preds.data_ptr(), target.data_ptr(), out.data_ptr(), B, C, H, W, _stream_ptr(preds.device)))
        return out

    @_on_engine_device
    def dft2(self, x: torch.Tensor, inverse: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
        """The 2-D transform of the engine on its own (include/xsd.h: xsd_fsim_test_dft2): x [B, n1, n2, 2] fp32 (re, im) ->
        torch.fft.fft2 / ifft2 of it in the same layout (into `out` if given)."""
        self._mine(x, "x")
        if x.dim() != 4 or x.shape[-1] != 2:
            raise XsdError(f"expected [B, n1, n2, 2] (re, im), got {tuple(x.shape)}")
        out = _out_like(out, x.shape, x.device, "out")
        B, n1, n2, _ = x.shape
        check(self.L.xsd_fsim_test_dft2(self.h, x.data_ptr(), out.data_ptr(), B, n1, n2, int(bool(inverse)), _stream_ptr(x.device)))
        return out

    # the regions xsd_fsim_test_stage copies out (include/xsd.h: XSD_FSIM_STAGE_*)
    STAGES = ("pooled", "eo", "en", "an", "a0sq", "T", "part", "filt", "noise")

    @_on_engine_device
    def stage(self, name: str, out: torch.Tensor | None = None):
        """One region of the last eval's workspace or plan (include/xsd.h: xsd_fsim_test_stage) -> (tensor, info): "pooled" float64
        [2B, h, w]; "eo" fp32 [2B, 16, h, w, 2]; "en", "an" float64 and "a0sq" fp32 [2B, 4, h, w]; "T" float64 [2B, 4]; "part" float64
        [B, ntiles, 2]; "filt" float64 [16, h, w]; "noise" float64 [3, 4].  info: dict(B = the leading count, h, w, entries, tiles_x,
        ntiles, tile_h, tile_w).  The copy goes into `out` (a contiguous device tensor of the region's dtype, at least its size) if given."""
        if name not in self.STAGES:
            raise XsdError(f"unknown stage {name!r} (one of {self.STAGES})")
        f32, f64 = torch.float32, torch.float64

        def layout(i):
            n, h, w = i[0], i[1], i[2]
            return {"pooled": (f64, (n, h, w)), "eo": (f32, (n, 16, h, w, 2)), "en": (f64, (n, 4, h, w)), "an": (f64, (n, 4, h, w)),
                    "a0sq": (f32, (n, 4, h, w)), "T": (f64, (n, 4)), "part": (f64, (n, i[5], 2)), "filt": (f64, (16, h, w)),
                    "noise": (f64, (3, 4))}[name]
        dev = torch.device("cuda", self.device_index)
        return _copy_stage(lambda ptr, nbytes, info: self.L.xsd_fsim_test_stage(self.h, self.STAGES.index(name), ptr, nbytes, info, _stream_ptr(dev)),
                           out, dev, layout)


@_on_tensor_device
def fsim_median(rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The exact selection of the fsim engine on its own (include/xsd.h: xsd_fsim_test_median): rows [R, n] fp32 -> [R], per row the
    element torch.median picks (NaN for a row that holds a NaN), into `out` if given."""
    _require_cuda_f32(rows, "rows")
    if rows.dim() != 2:
        raise XsdError(f"expected [rows, n], got {tuple(rows.shape)}")
    out = _out_like(out, (rows.shape[0],), rows.device, "out")
    check(_lib.load().xsd_fsim_test_median(rows.data_ptr(), out.data_ptr(), int(rows.shape[0]), int(rows.shape[1]), _stream_ptr(rows.device)))
    return out


def fft_size_supported(n: int) -> bool:
    """csrc/swinfir.hip: the FourierUnit's FFT takes lengths up to 4096 whose prime factors are all <= 13"""
    return bool(_lib.load().xsd_swinfir_fft_supported(int(n)))


# ---- stateless transform entry points --------------------------------------------------------------------------
@_on_tensor_device
def mask_pad_normalize(counts: torch.Tensor, mask: torch.Tensor | None, res: int, max_val: float | None,
                       stretch: str = "linear") -> torch.Tensor:
    """counts [B,Hin,Win] int32|float32 (CUDA), mask [Hin,Win] uint8 -> [B,1,res,res] float32."""
    L = _lib.load()
    if not counts.is_cuda:
        raise XsdError("counts must be a CUDA(HIP) tensor: no CPU fallback")
    if counts.dtype not in (torch.int32, torch.float32) or not counts.is_contiguous():
        raise XsdError("counts must be contiguous int32 or float32")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_cuda or tuple(mask.shape) != tuple(counts.shape[-2:])):
        raise XsdError("mask must be a CUDA uint8 tensor [Hin,Win]")
    B, Hin, Win = counts.shape
    out = torch.empty((B, 1, res, res), device=counts.device, dtype=torch.float32)
    check(L.xsd_mask_pad_normalize(counts.data_ptr(), int(counts.dtype == torch.int32),
                                   mask.data_ptr() if mask is not None else None, out.data_ptr(), B, Hin, Win, res,
                                   int(max_val is not None), float(max_val or 0.0), STRETCH[stretch],
                                   _stream_ptr(counts.device)))
    return out


@_on_tensor_device
def compose_input(img: torch.Tensor, agn: torch.Tensor | None, bkg: torch.Tensor | None, mask: torch.Tensor | None,
                  res: int, max_val: float | None, stretch: str = "linear", upsample: int = 1,
                  big_endian: bool = False) -> torch.Tensor:
    """One-kernel sample composition (include/xsd.h: xsd_compose_input): img (+agn) (+bkg) -> * mask -> optional nearest
    upsample / s^2 -> centred pad to res -> optional normalize.  img/agn/bkg: [B,Hin,Win] int32 or float32 (CUDA); with
    big_endian=True they hold raw FITS words (e.g. torch.frombuffer of the HDU data block viewed as int32)."""
    L = _lib.load()
    for n, t in (("img", img), ("agn", agn), ("bkg", bkg)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != img.dtype or tuple(t.shape) != tuple(img.shape) or not t.is_contiguous():
            raise XsdError(f"{n} must be a contiguous CUDA tensor with img's dtype and shape")
    if img.dtype not in (torch.int32, torch.float32):
        raise XsdError("img must be int32 or float32")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_cuda or tuple(mask.shape) != tuple(img.shape[-2:])):
        raise XsdError("mask must be a CUDA uint8 tensor [Hin,Win]")
    B, Hin, Win = img.shape
    out = torch.empty((B, 1, res, res), device=img.device, dtype=torch.float32)
    check(L.xsd_compose_input(img.data_ptr(), agn.data_ptr() if agn is not None else None,
                              bkg.data_ptr() if bkg is not None else None, int(img.dtype == torch.int32), int(big_endian),
                              mask.data_ptr() if mask is not None else None, out.data_ptr(), B, Hin, Win, int(upsample), res,
                              int(max_val is not None), float(max_val or 0.0), STRETCH[stretch], _stream_ptr(img.device)))
    return out


@_on_tensor_device
def compose_batch(pool: torch.Tensor, img_idx, agn_idx, bkg_idx, mask: torch.Tensor | None, Hin: int, Win: int, res: int,
                  max_val: float | None, stretch: str = "linear", upsample: int = 1, is_int32: bool = True,
                  big_endian: bool = True) -> torch.Tensor:
    """Batched gather-compose (include/xsd.h: xsd_compose_batch): pool [n_slots, slot_elems] int32 (CUDA) of raw FITS data
    blocks; img_idx / agn_idx / bkg_idx: host int32 sequences of B slot numbers (agn / bkg: -1 = absent, None = absent for all).
    Returns [B,1,res,res] float32, bitwise equal to compose_input on the same slots stacked by hand."""
    import numpy as np
    L = _lib.load()
    if not pool.is_cuda or pool.dtype != torch.int32 or pool.dim() != 2 or not pool.is_contiguous():
        raise XsdError("pool must be a contiguous CUDA int32 tensor [n_slots, slot_elems]")
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_cuda or tuple(mask.shape) != (Hin, Win)):
        raise XsdError("mask must be a CUDA uint8 tensor [Hin,Win]")
    idx = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (img_idx, agn_idx, bkg_idx)]
    B = int(idx[0].size)
    for n, a in zip(("agn", "bkg"), idx[1:]):
        if a is not None and a.size != B:
            raise XsdError(f"{n}_idx holds {a.size} entries for {B} samples")
    out = torch.empty((B, 1, res, res), device=pool.device, dtype=torch.float32)
    ptr = [None if a is None else a.ctypes.data for a in idx]
    check(L.xsd_compose_batch(pool.data_ptr(), int(is_int32), int(big_endian), pool.shape[1], pool.shape[0], ptr[0], ptr[1], ptr[2],
                              mask.data_ptr() if mask is not None else None, out.data_ptr(), B, Hin, Win, int(upsample), res,
                              int(max_val is not None), float(max_val or 0.0), STRETCH[stretch], _stream_ptr(pool.device)))
    return out


@_on_tensor_device
def normalize(img: torch.Tensor, max_val: float, stretch: str, inverse: bool = False) -> torch.Tensor:
    L = _lib.load()
    _require_cuda_f32(img, "img")
    out = torch.empty_like(img)
    check(L.xsd_normalize(img.data_ptr(), out.data_ptr(), img.numel(), float(max_val), STRETCH[stretch], int(inverse),
                          _stream_ptr(img.device)))
    return out


@_on_tensor_device
def image_upsample(x: torch.Tensor, scale: int) -> torch.Tensor:
    L = _lib.load()
    _require_cuda_f32(x, "x")
    H, W = x.shape[-2:]
    n = x.numel() // (H * W)
    out = torch.empty(tuple(x.shape[:-2]) + (H * scale, W * scale), device=x.device, dtype=torch.float32)
    check(L.xsd_image_upsample(x.data_ptr(), out.data_ptr(), n, H, W, scale, _stream_ptr(x.device)))
    return out
