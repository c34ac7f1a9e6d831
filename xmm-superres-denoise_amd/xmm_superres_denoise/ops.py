"""The four operations of the Swin-family engines as differentiable torch ops on hand-written HIP (include/xsd.h, "differentiable Swin
ops"; csrc/sw_ops.hip): `linear`, `conv3x3`, `layer_norm` and `window_attention`.  Each is a torch.autograd.Function over one forward
and one backward entry of the library; a trainable network composes them in Python and torch's autograd holds the graph
(models/modules/swinir_train.py).

All take contiguous fp32 CUDA tensors, run asynchronously on the current stream of their first tensor's device, and allocate their
scratch through torch.  fp32 only ("bf16x6" is refused by name).  The backward is once-differentiable: a second differentiation is
refused.  Where no input needs a gradient (torch.no_grad(), torch.inference_mode(), frozen inputs) nothing is saved, and the forward of
layer_norm and window_attention is the SAME kernel with the SAME arguments as engine.sw_layernorm / sw_window_attention: the results are
bitwise theirs.  linear and conv3x3 are NOT engine.sw_gemm's kernel: they carry the whole sum over K and the bias in double and round
once (csrc/sw_ops.hip says why), so they agree with sw_gemm / sw_conv3x3 to rounding, not bit for bit.
With a gradient and an activation, the GEMM stores the pre-activation and a second kernel applies the epilogue's own expression to it:
the same bits as the fused epilogue, at the price of one more [M, N] tensor kept for the backward (the derivative of GELU / LeakyReLU
needs it; recomputing it would cost the whole GEMM again).

What is saved: linear / conv3x3: the input, the weight and, with an activation, the pre-activation.  layer_norm: the input and the
weight (mean and variance are recomputed in double).  window_attention: qkv and the table (the probabilities are recomputed; no
ws^2 x ws^2 matrix is kept).

HAT's two operations on top of them (include/xsd.h, "differentiable HAT ops"; csrc/hat_ops.hip), under the same rules:
`overlap_attention`, the overlapping cross-attention of the OCAB (the kernel of engine.hat_ocab_attention: the same bits; saves qkv,
the table and its output, from which the backward takes delta = dout . out; no ws^2 x ow^2 matrix is kept), and `channel_attention`,
the gate at the end of the CAB (the gates are bitwise those of engine.hat_ca_combine; saves its input and the four weights; the
backward recomputes the mean, the hidden vector and the gate in double, so the fp32 gate's rounding does not reach dt).
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .engine import XsdError, _lib
from .engine._lib import check
from .engine.engine import SW_ACT, _require_cuda_f32, _stream_ptr

__all__ = ["linear", "conv3x3", "layer_norm", "window_attention", "overlap_attention", "channel_attention", "LRELU_SLOPE"]

LRELU_SLOPE = 0.01           # nn.LeakyReLU's default, what engine.sw_gemm's "lrelu" runs


def _needs_grad(ctx, grad_mode: bool) -> bool:
    # needs_input_grad mirrors requires_grad whatever the grad mode, and inside Function.forward the grad mode is always off: the
    # wrappers below pass the caller's.  Under no_grad / inference_mode nothing is to be saved.
    return grad_mode and any(ctx.needs_input_grad)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _math(math: str) -> int:
    if math == "bf16x6":
        raise XsdError("math mode 'bf16x6' is not supported by the differentiable ops (fp32 only)")
    if math != "fp32":
        raise XsdError(f"unknown math mode {math!r}: the differentiable ops run in 'fp32' only")
    return 0


def _act(act):
    if act not in SW_ACT:
        raise XsdError(f"unknown activation {act!r}: {list(SW_ACT)}")
    return SW_ACT[act]


def _scratch(nbytes: int, device) -> torch.Tensor:
    if nbytes < 0:
        raise XsdError(f"libxsd_hip: {_lib.load().xsd_last_error().decode()}")
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _check_bias(bias, N):
    if bias is not None:
        _require_cuda_f32(bias, "bias")
        if bias.numel() != N:
            raise XsdError(f"bias has {bias.numel()} elements for {N} outputs")


class _GemmFn(torch.autograd.Function):
    """linear (conv = False: a [M, K], w [N, K]) and conv3x3 (conv = True: a [B, H, W, cin], w [N, cin, 3, 3])"""

    @staticmethod
    def forward(ctx, a, w, bias, conv, act, slope, chunk, grad_mode):
        L = _lib.load()
        N = int(w.shape[0])
        need = _needs_grad(ctx, grad_mode)
        with torch.cuda.device(a.device):
            y = torch.empty(tuple(a.shape[:-1]) + (N,), device=a.device, dtype=torch.float32)
            z = torch.empty_like(y) if need and act else None
            st = _stream_ptr(a.device)
            if conv:
                B, H, W, cin = (int(v) for v in a.shape)
                dims = (B, H, W, cin, N)
                s = _scratch(L.xsd_sw_op_conv3x3_scratch(*dims, act, 0, 0), a.device)
                check(L.xsd_sw_op_conv3x3_forward(a.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(z), *dims, act, slope, 0,
                                                  s.data_ptr(), s.numel(), st))
            else:
                dims = (int(a.shape[0]), int(a.shape[1]), N)
                s = _scratch(L.xsd_sw_op_linear_scratch(*dims, act, 0, 0), a.device)
                check(L.xsd_sw_op_linear_forward(a.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(z), *dims, act, slope, 0,
                                                 s.data_ptr(), s.numel(), st))
        if need:
            ctx.save_for_backward(a, w, z)
            ctx.cfg = (conv, dims, act, slope, chunk, bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a, w, z = ctx.saved_tensors
        conv, dims, act, slope, chunk, has_bias = ctx.cfg
        L = _lib.load()
        dy = dy.contiguous()
        _require_cuda_f32(dy, "dy")
        with torch.cuda.device(a.device):
            da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
            dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
            db = torch.empty(dims[-1], device=a.device, dtype=torch.float32) if has_bias and ctx.needs_input_grad[2] else None
            st = _stream_ptr(a.device)
            if conv:
                s = _scratch(L.xsd_sw_op_conv3x3_scratch(*dims, act, chunk, 1), a.device)
                check(L.xsd_sw_op_conv3x3_backward(dy.data_ptr(), a.data_ptr(), w.data_ptr(), _ptr(z), _ptr(da), _ptr(dw), _ptr(db), *dims, act,
                                                   slope, 0, chunk, s.data_ptr(), s.numel(), st))
            else:
                s = _scratch(L.xsd_sw_op_linear_scratch(*dims, act, chunk, 1), a.device)
                check(L.xsd_sw_op_linear_backward(dy.data_ptr(), a.data_ptr(), w.data_ptr(), _ptr(z), _ptr(da), _ptr(dw), _ptr(db), *dims, act,
                                                  slope, 0, chunk, s.data_ptr(), s.numel(), st))
        return da, dw, db, None, None, None, None, None


def linear(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None, slope: float = LRELU_SLOPE,
           chunk: int = 0, math: str = "fp32") -> torch.Tensor:
    """act(a w^T + bias): a [..., K] token rows, w [N, K] as a Linear stores it -> [..., N]; act None, "gelu" (exact erf) or "lrelu"
    (LeakyReLU(slope)).  Gradients: a, w, bias.  `chunk`: token rows per weight-gradient partial (0: the library's choice); the
    partials are summed in ascending order."""
    _math(math)
    act = _act(act)
    _require_cuda_f32(a, "a")
    _require_cuda_f32(w, "w")
    if a.dim() < 2 or w.dim() != 2 or a.shape[-1] != w.shape[1]:
        raise XsdError(f"a {tuple(a.shape)} and w {tuple(w.shape)} are not [..., K] and [N, K]")
    _check_bias(bias, int(w.shape[0]))
    y = _GemmFn.apply(a.reshape(-1, a.shape[-1]), w, bias, False, act, float(slope), int(chunk), torch.is_grad_enabled())
    return y.view(tuple(a.shape[:-1]) + (int(w.shape[0]),))


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, act: str | None = None, slope: float = LRELU_SLOPE,
            chunk: int = 0, math: str = "fp32") -> torch.Tensor:
    """act(conv3x3(x) + bias), zero padding 1: x [B, H, W, cin] token-major, w [N, cin, 3, 3] as a Conv2d stores it -> [B, H, W, N]
    token-major.  Gradients: x, w, bias."""
    _math(math)
    act = _act(act)
    _require_cuda_f32(x, "x")
    _require_cuda_f32(w, "w")
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (x.shape[3], 3, 3):
        raise XsdError(f"x {tuple(x.shape)} and w {tuple(w.shape)} are not [B, H, W, cin] and [N, cin, 3, 3]")
    _check_bias(bias, int(w.shape[0]))
    return _GemmFn.apply(x, w, bias, True, act, float(slope), int(chunk), torch.is_grad_enabled())


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, grad_mode):
        L = _lib.load()
        M, C = (int(v) for v in x.shape)
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(L.xsd_sw_op_layernorm_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, C, _stream_ptr(x.device)))
        if _needs_grad(ctx, grad_mode):
            ctx.save_for_backward(x, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        L = _lib.load()
        M, C = (int(v) for v in x.shape)
        dy = dy.contiguous()
        _require_cuda_f32(dy, "dy")
        with torch.cuda.device(x.device):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            wb = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
            dw = torch.empty_like(w) if wb else None
            db = torch.empty_like(w) if wb else None
            s = _scratch(L.xsd_sw_op_layernorm_scratch(M, C), x.device)
            check(L.xsd_sw_op_layernorm_backward(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db), M, C, s.data_ptr(),
                                                 s.numel(), _stream_ptr(x.device)))
        return dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(x - mean) / sqrt(var + 1e-5) * w + b over the last dimension (biased variance, statistics in double): x [..., C], w and b [C].
    Gradients: x, w, b."""
    for n, t in (("x", x), ("w", w), ("b", b)):
        _require_cuda_f32(t, n)
    if x.dim() < 2 or w.numel() != x.shape[-1] or b.numel() != x.shape[-1]:
        raise XsdError(f"x {tuple(x.shape)}, w {tuple(w.shape)} and b {tuple(b.shape)} are not [..., C], [C] and [C]")
    return _LayerNormFn.apply(x.reshape(-1, x.shape[-1]), w, b, torch.is_grad_enabled()).view(x.shape)


class _WindowAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, H, W, heads, ws, shift, scale, grad_mode):
        L = _lib.load()
        B, _, C3 = (int(v) for v in qkv.shape)
        with torch.cuda.device(qkv.device):
            out = torch.empty((B, H * W, C3 // 3), device=qkv.device, dtype=torch.float32)
            check(L.xsd_sw_op_attention_forward(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, C3 // 3, heads, ws, shift, scale,
                                                _stream_ptr(qkv.device)))
        if _needs_grad(ctx, grad_mode):
            ctx.save_for_backward(qkv, table)
            ctx.cfg = (B, H, W, C3 // 3, heads, ws, shift, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, table = ctx.saved_tensors
        B, H, W, C, heads, ws, shift, scale = ctx.cfg
        L = _lib.load()
        dout = dout.contiguous()
        _require_cuda_f32(dout, "dout")
        with torch.cuda.device(qkv.device):
            dqkv, dtable = torch.empty_like(qkv), torch.empty_like(table)
            s = _scratch(L.xsd_sw_op_attention_scratch(B, H, W, C, heads, ws), qkv.device)
            check(L.xsd_sw_op_attention_backward(dout.data_ptr(), qkv.data_ptr(), table.data_ptr(), dqkv.data_ptr(), dtable.data_ptr(), B, H, W, C,
                                                 heads, ws, shift, scale, s.data_ptr(), s.numel(), _stream_ptr(qkv.device)))
        return dqkv, dtable, None, None, None, None, None, None, None


def window_attention(qkv: torch.Tensor, table: torch.Tensor, H: int, W: int, heads: int, ws: int, shift: int, scale: float) -> torch.Tensor:
    """The shifted-window attention between the qkv Linear and proj: qkv [B, H W, 3 C] token rows in image order, table
    [(2 ws - 1)^2, heads] -> [B, H W, C] in image order, with the roll by -shift, the window partition and the -100 shift mask of the
    run-time size.  ws 1..16, at most 32 channels per head.  Gradients: qkv and table."""
    _require_cuda_f32(qkv, "qkv")
    _require_cuda_f32(table, "table")
    if qkv.dim() != 3 or qkv.shape[1] != H * W or qkv.shape[2] % 3 or tuple(table.shape) != ((2 * ws - 1) ** 2, heads):
        raise XsdError(f"qkv {tuple(qkv.shape)} / table {tuple(table.shape)} do not fit {H} x {W}, {heads} heads, window {ws}")
    return _WindowAttentionFn.apply(qkv, table, int(H), int(W), int(heads), int(ws), int(shift), float(scale), torch.is_grad_enabled())


class _OverlapAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, H, W, heads, ws, ow, scale, grad_mode):
        L = _lib.load()
        B, _, C3 = (int(v) for v in qkv.shape)
        with torch.cuda.device(qkv.device):
            out = torch.empty((B, H * W, C3 // 3), device=qkv.device, dtype=torch.float32)
            check(L.xsd_hat_op_ocab_forward(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, C3 // 3, heads, ws, ow, scale,
                                            _stream_ptr(qkv.device)))
        if _needs_grad(ctx, grad_mode):
            ctx.save_for_backward(qkv, table, out)
            ctx.cfg = (B, H, W, C3 // 3, heads, ws, ow, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, table, out = ctx.saved_tensors
        B, H, W, C, heads, ws, ow, scale = ctx.cfg
        L = _lib.load()
        dout = dout.contiguous()
        _require_cuda_f32(dout, "dout")
        with torch.cuda.device(qkv.device):
            dqkv, dtable = torch.empty_like(qkv), torch.empty_like(table)
            s = _scratch(L.xsd_hat_op_ocab_scratch(B, H, W, C, heads, ws, ow), qkv.device)
            check(L.xsd_hat_op_ocab_backward(dout.data_ptr(), qkv.data_ptr(), table.data_ptr(), out.data_ptr(), dqkv.data_ptr(), dtable.data_ptr(),
                                             B, H, W, C, heads, ws, ow, scale, s.data_ptr(), s.numel(), _stream_ptr(qkv.device)))
        return dqkv, dtable, None, None, None, None, None, None, None


def overlap_attention(qkv: torch.Tensor, table: torch.Tensor, H: int, W: int, heads: int, ws: int, ow: int, scale: float) -> torch.Tensor:
    """The overlapping cross-attention of HAT's OCAB between its qkv Linear and proj: qkv [B, H W, 3 C] token rows in image order, table
    [(ws + ow - 1)^2, heads] -> [B, H W, C] in image order.  The ws x ws queries of a window attend to the ow x ow keys / values of the
    overlapping window around it (stride ws, zero padding (ow - ws) / 2); a key outside the image is a zero vector that stays in the
    softmax with score = bias; the bias index is the reference's, negative entries wrapping.  ws 1..16, ws <= ow <= 32, ow - ws even, at
    most 32 channels per head.  Gradients: qkv and table."""
    _require_cuda_f32(qkv, "qkv")
    _require_cuda_f32(table, "table")
    if qkv.dim() != 3 or qkv.shape[1] != H * W or qkv.shape[2] % 3 or tuple(table.shape) != ((ws + ow - 1) ** 2, heads):
        raise XsdError(f"qkv {tuple(qkv.shape)} / table {tuple(table.shape)} do not fit {H} x {W}, {heads} heads, window {ws}, overlap window {ow}")
    return _OverlapAttentionFn.apply(qkv, table, int(H), int(W), int(heads), int(ws), int(ow), float(scale), torch.is_grad_enabled())


class _ChannelAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, w1, b1, w2, b2, grad_mode):
        L = _lib.load()
        B, HW, C = (int(v) for v in t.shape)
        Cs = int(b1.numel())
        with torch.cuda.device(t.device):
            y = torch.empty_like(t)
            s = _scratch(L.xsd_hat_op_ca_scratch(B, HW, C, Cs, 0), t.device)
            check(L.xsd_hat_op_ca_forward(t.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), None,
                                          B, HW, C, Cs, s.data_ptr(), s.numel(), _stream_ptr(t.device)))
        if _needs_grad(ctx, grad_mode):
            ctx.save_for_backward(t, w1, b1, w2, b2)
            ctx.cfg = (B, HW, C, Cs)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        t, w1, b1, w2, b2 = ctx.saved_tensors
        B, HW, C, Cs = ctx.cfg
        L = _lib.load()
        dy = dy.contiguous()
        _require_cuda_f32(dy, "dy")
        with torch.cuda.device(t.device):
            dt, dw1, db1, dw2, db2 = (torch.empty_like(v) for v in (t, w1, b1, w2, b2))
            s = _scratch(L.xsd_hat_op_ca_scratch(B, HW, C, Cs, 1), t.device)
            check(L.xsd_hat_op_ca_backward(dy.data_ptr(), t.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dt.data_ptr(),
                                           dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), B, HW, C, Cs,
                                           s.data_ptr(), s.numel(), _stream_ptr(t.device)))
        return tuple(g if need else None for g, need in zip((dt, dw1, db1, dw2, db2), ctx.needs_input_grad)) + (None,)


def channel_attention(t: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """The channel attention at the end of HAT's CAB: t [B, HW, C] (or [B, H, W, C]) token-major -> t * g[b, c] with
    g = sigmoid(w2 relu(w1 mean_p t + b1) + b2); w1 [Cs, C, 1, 1] and w2 [C, Cs, 1, 1] as the 1x1 Conv2ds store them (or [Cs, C] and
    [C, Cs]), b1 [Cs], b2 [C].  The mean is a double sum over chunks of 256 pixels in a fixed order.  Gradients: all five."""
    for n, v in (("t", t), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        _require_cuda_f32(v, n)
    C, Cs = int(t.shape[-1]), int(b1.numel())
    if t.dim() not in (3, 4) or w1.numel() != Cs * C or w2.numel() != C * Cs or b2.numel() != C or w1.shape[0] != Cs or w2.shape[0] != C:
        raise XsdError(f"t {tuple(t.shape)}, w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, w2 {tuple(w2.shape)}, b2 {tuple(b2.shape)} are not "
                       f"[B, HW, C] and a squeeze MLP of {C} channels")
    y = _ChannelAttentionFn.apply(t.reshape(t.shape[0], -1, C), w1, b1, w2, b2, torch.is_grad_enabled())
    return y.view(t.shape)
