"""The differentiable Swin ops (include/xsd.h "differentiable Swin ops", csrc/sw_ops.hip, xmm_superres_denoise/ops.py): linear, conv3x3,
layer_norm and window_attention, forward and backward, each against torch's autograd of a plain float64 restatement.  The yardstick is
the project's (test_hip_sw_kernels._assert_within_2x_of_fp32): for every compared tensor the engine's error against float64 is at most
twice that of the same restatement in fp32 through torch autograd on the same device, in rms and in max |err| relative to the tensor's
max -- and the yardstick's own error must be non-zero, so that a bar of 0 neither passes nor fails by accident.  The one case where the
fp32 yardstick is exact by construction (a window of one token: the softmax is 1, the score gradient 0) is held to exactness instead.

The library entries are called directly with NaN-filled outputs and sentinel guards behind them; the autograd Functions of ops.py are
then held bit for bit to those calls, and in eval to engine.sw_layernorm / sw_window_attention."""
import pytest
import torch
import torch.nn.functional as F

import swinfir_torch as st
from test_hip_sw_kernels import ATTN_CASES, _assert_within_2x_of_fp32, _attn_inputs, _guarded, _ln_params, _untouched

pytestmark = pytest.mark.gpu
ACT = {None: 0, "gelu": 1, "lrelu": 2}
SLOPE = 0.01


def _bar(y, y32, y64, what):
    rms32 = _assert_within_2x_of_fp32(y, y32, y64, what)
    assert rms32 > 0, (what, "the fp32 yardstick is exact here: a bar of 0 proves nothing")
    return rms32


def _lib():
    from xmm_superres_denoise.engine import _lib
    return _lib.load()


def _p(t):
    return t.data_ptr() if t is not None else None


def _scratch(nbytes):
    assert nbytes >= 0, _lib().xsd_last_error()
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _act64(z, act):
    return z if act is None else (F.gelu(z) if act == "gelu" else F.leaky_relu(z, SLOPE))


# ---------------------------------------------------------------------------------------------------------------
# linear / conv3x3 through the library, outputs guarded
# ---------------------------------------------------------------------------------------------------------------
def _lib_gemm(a, w, b, act, dy, chunk=0, conv=False, want=(True, True, True)):
    """-> y, da, dw, db of the library's forward + backward entries; every output NaN-filled with sentinels behind it"""
    L = _lib()
    N = int(w.shape[0])
    dims = tuple(int(v) for v in a.shape) + (N,)
    name = "conv3x3" if conv else "linear"
    fwd, bwd, scr = (getattr(L, f"xsd_sw_op_{name}_{k}") for k in ("forward", "backward", "scratch"))
    outs = [_guarded(tuple(a.shape[:-1]) + (N,)), _guarded(tuple(a.shape[:-1]) + (N,)) if act else (None, None),
            _guarded(tuple(a.shape)) if want[0] else (None, None), _guarded(tuple(w.shape)) if want[1] else (None, None),
            _guarded((N,)) if want[2] and b is not None else (None, None)]
    (y, _), (z, _), (da, _), (dw, _), (db, _) = outs
    s = _scratch(scr(*dims, ACT[act], 0, 0))
    rc = fwd(a.data_ptr(), w.data_ptr(), _p(b), y.data_ptr(), _p(z), *dims, ACT[act], SLOPE, 0, s.data_ptr(), s.numel(), _stream())
    assert rc == 0, L.xsd_last_error()
    s = _scratch(scr(*dims, ACT[act], chunk, 1))
    rc = bwd(dy.data_ptr(), a.data_ptr(), w.data_ptr(), _p(z), _p(da), _p(dw), _p(db), *dims, ACT[act], SLOPE, 0, chunk, s.data_ptr(), s.numel(),
             _stream())
    assert rc == 0, L.xsd_last_error()
    torch.cuda.synchronize()
    for t, g in outs:
        if t is not None:
            assert _untouched(g) and (torch.isfinite(t).all() or not torch.isfinite(dy).all())
    return y, da, dw, db


def _ref_gemm(a, w, b, act, dy, conv, dtype):
    a, w, dy = (t.to(dtype).detach().requires_grad_(r) for t, r in ((a, True), (w, True), (dy, False)))
    b = b.to(dtype).detach().requires_grad_(True) if b is not None else None
    if conv:
        z = F.conv2d(F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1)), w, b).permute(0, 2, 3, 1)      # the zero pad made: a 1 x 1 image is no NHWC / NCHW riddle
    else:
        z = F.linear(a, w, b)
    y = _act64(z, act)
    y.backward(dy)
    return y.detach(), a.grad, w.grad, b.grad if b is not None else None


def _check_gemm(a, w, b, act, dy, what, chunk=0, conv=False):
    got = _lib_gemm(a, w, b, act, dy, chunk, conv)
    r64, r32 = _ref_gemm(a, w, b, act, dy, conv, torch.float64), _ref_gemm(a, w, b, act, dy, conv, torch.float32)
    for n, g, y32, y64 in zip(("y", "da", "dw", "db"), got, r32, r64):
        if g is not None:
            _bar(g, y32, y64, f"{what}: {n}")
    return got


def _lin_inputs(M, K, N, bias, seed=0):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * K + N + seed)
    a = torch.randn(M, K, generator=g).cuda()
    w = ((torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5).cuda()
    b = (torch.rand(N, generator=g) - 0.5).cuda() if bias else None
    return a, w, b, torch.randn(M, N, generator=g).cuda()


@pytest.mark.parametrize("act", [None, "gelu", "lrelu"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("K,N", [(10, 12), (36, 70), (180, 540)])
def test_linear_against_float64(K, N, bias, act):
    """480 rows = 2 x 12 x 20 (no multiple of the 128-row tile); the weight gradient in chunks of 112 rows, which do not divide 480"""
    a, w, b, dy = _lin_inputs(480, K, N, bias)
    _check_gemm(a, w, b, act, dy, f"linear 480 x {K} -> {N}, bias {bias}, act {act}", chunk=112)


def test_linear_of_one_row():
    """M = 1 (with GELU: without an activation db = dy and da, dw are single products, which fp32 torch gets exactly)"""
    a, w, b, dy = _lin_inputs(1, 36, 70, True)
    _check_gemm(a, w, b, "gelu", dy, "linear 1 x 36 -> 70, gelu")


CONV_CASES = [(cin, cout, H, W) for cin, cout in ((1, 6), (6, 6), (5, 1), (12, 70)) for H, W in ((1, 1), (5, 7), (17, 45))]


def _conv_inputs(B, H, W, cin, cout, seed=0):
    g = torch.Generator().manual_seed(100003 * H + 1009 * W + 31 * cin + cout + seed)
    x = torch.randn(B, H, W, cin, generator=g).cuda()
    w = ((torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (9 * cin) ** 0.5).cuda()
    b = (torch.rand(cout, generator=g) - 0.5).cuda()
    return x, w, b, torch.randn(B, H, W, cout, generator=g).cuda()


@pytest.mark.parametrize("i,case", list(enumerate(CONV_CASES)))
def test_conv3x3_against_float64(i, case):
    cin, cout, H, W = case
    act = (None, "gelu", "lrelu")[i % 3]
    # 5 -> 1 on a 1 x 1 image without an activation: db is the single addition dy[0] + dy[1], which seed 0 happens to draw exactly
    # representable (a yardstick of 0); seed 1 draws a sum that fp32 has to round
    x, w, b, dy = _conv_inputs(2, H, W, cin, cout, seed=1 if (cin, cout, H, W) == (5, 1, 1, 1) else 0)
    _check_gemm(x, w, b, act, dy, f"conv3x3 2 x {H} x {W}, {cin} -> {cout}, act {act}", chunk=(0, 100)[i % 2], conv=True)


@pytest.mark.parametrize("conv", [False, True])
def test_gemm_ops_are_reproducible_batch_independent_and_keep_a_nan_in_its_image(conv):
    if conv:
        x, w, b, dy = _conv_inputs(2, 17, 45, 12, 70)
    else:
        x, w, b, dy = _lin_inputs(480, 36, 70, True)
        x, dy = x.view(2, 240, 36), dy.view(2, 240, 70)

    def run(x, dy):
        if conv:
            return _lib_gemm(x, w, b, "gelu", dy, 0, True)
        y, da, dw, db = _lib_gemm(x.reshape(-1, 36), w, b, "gelu", dy.reshape(-1, 70), 0, False)
        return y.view(dy.shape), da.view(x.shape), dw, db
    first, again = run(x, dy), run(x, dy)
    for p, q in zip(first, again):
        assert torch.equal(p, q)                                       # two runs: bit for bit
    for i in range(2):
        y1, dx1, _, _ = run(x[i:i + 1].contiguous(), dy[i:i + 1].contiguous())
        assert torch.equal(y1[0], first[0][i]) and torch.equal(dx1[0], first[1][i]), i
    bad = dy.clone()
    bad[1].view(-1)[777] = float("nan")
    _, dxn, _, _ = run(x, bad)
    assert torch.equal(dxn[0], first[1][0]) and not torch.isfinite(dxn[1]).all()


# ---------------------------------------------------------------------------------------------------------------
# layer_norm
# ---------------------------------------------------------------------------------------------------------------
def _lib_ln(x, w, b, dy, want_dx=True, want_wb=True):
    L = _lib()
    M, C = (int(v) for v in x.shape)
    outs = [_guarded((M, C)), _guarded((M, C)) if want_dx else (None, None), _guarded((C,)) if want_wb else (None, None),
            _guarded((C,)) if want_wb else (None, None)]
    (y, _), (dx, _), (dw, _), (db, _) = outs
    assert L.xsd_sw_op_layernorm_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, C, _stream()) == 0, L.xsd_last_error()
    s = _scratch(L.xsd_sw_op_layernorm_scratch(M, C))
    rc = L.xsd_sw_op_layernorm_backward(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _p(dx), _p(dw), _p(db), M, C, s.data_ptr(), s.numel(), _stream())
    assert rc == 0, L.xsd_last_error()
    torch.cuda.synchronize()
    for t, g in outs:
        if t is not None:
            assert _untouched(g) and (torch.isfinite(t).all() or not torch.isfinite(dy).all())
    return y, dx, dw, db


def _ref_ln(x, w, b, dy, dtype):
    x, w, b = (t.to(dtype).detach().requires_grad_(True) for t in (x, w, b))
    y = F.layer_norm(x, (x.shape[-1],), w, b, eps=1e-5)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, w.grad, b.grad


def _check_ln(x, w, b, dy, what):
    got = _lib_ln(x, w, b, dy)
    r64, r32 = _ref_ln(x, w, b, dy, torch.float64), _ref_ln(x, w, b, dy, torch.float32)
    for n, g, y32, y64 in zip(("y", "dx", "dw", "db"), got, r32, r64):
        _bar(g, y32, y64, f"{what}: {n}")
    assert all(torch.equal(p, q) for p, q in zip(got, _lib_ln(x, w, b, dy)))             # two runs: bit for bit
    return got


@pytest.mark.parametrize("M,C", [(37, 6), (5, 180), (7, 65), (3, 2), (2, 4096), (300, 24)])
def test_layer_norm_against_float64(M, C):
    """(300, 24): more than one 128-row partial of the weight gradient, the last one short"""
    g = torch.Generator().manual_seed(1000 * M + C)
    x = (torch.randn(M, C, generator=g) * 3 + 0.7).cuda()
    w, b = _ln_params(C, g)
    _check_ln(x, w, b, torch.randn(M, C, generator=g).cuda(), f"layer_norm {M} x {C}")


def test_layer_norm_of_a_large_mean_with_a_small_spread():
    g = torch.Generator().manual_seed(77)
    x = (1000 + 1e-3 * torch.randn(64, 180, generator=g)).cuda()
    w, b = _ln_params(180, g)
    _check_ln(x, w, b, torch.randn(64, 180, generator=g).cuda(), "layer_norm 64 x 180, 1000 + 1e-3 randn")


def test_layer_norm_rows_are_independent_and_keep_a_nan():
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(2, 150, 65, generator=g).cuda(), torch.randn(2, 150, 65, generator=g).cuda()
    w, b = _ln_params(65, g)
    _, dx, _, _ = _lib_ln(x.view(-1, 65), w, b, dy.view(-1, 65))
    for i in range(2):
        _, d1, _, _ = _lib_ln(x[i], w, b, dy[i])
        assert torch.equal(d1, dx.view(2, 150, 65)[i]), i
    bad = dy.clone()
    bad[1, 3, 4] = float("nan")
    _, dxn, _, _ = _lib_ln(x.view(-1, 65), w, b, bad.view(-1, 65))
    assert torch.equal(dxn.view(2, 150, 65)[0], dx.view(2, 150, 65)[0]) and not torch.isfinite(dxn).all()
    _, only_dx, none_w, none_b = _lib_ln(x.view(-1, 65), w, b, dy.view(-1, 65), want_wb=False)
    assert none_w is None and none_b is None and torch.equal(only_dx, dx)


# ---------------------------------------------------------------------------------------------------------------
# window attention
# ---------------------------------------------------------------------------------------------------------------
def _lib_attn(qkv, table, dout, H, W, heads, ws, shift, scale):
    L = _lib()
    B, _, C3 = (int(v) for v in qkv.shape)
    C = C3 // 3
    outs = [_guarded((B, H * W, C)), _guarded((B, H * W, C3)), _guarded(tuple(table.shape))]
    (o, _), (dqkv, _), (dtable, _) = outs
    assert L.xsd_sw_op_attention_forward(qkv.data_ptr(), table.data_ptr(), o.data_ptr(), B, H, W, C, heads, ws, shift, scale, _stream()) == 0
    s = _scratch(L.xsd_sw_op_attention_scratch(B, H, W, C, heads, ws))
    rc = L.xsd_sw_op_attention_backward(dout.data_ptr(), qkv.data_ptr(), table.data_ptr(), dqkv.data_ptr(), dtable.data_ptr(), B, H, W, C, heads, ws,
                                        shift, scale, s.data_ptr(), s.numel(), _stream())
    assert rc == 0, L.xsd_last_error()
    torch.cuda.synchronize()
    for t, g in outs:
        assert _untouched(g) and (torch.isfinite(t).all() or not torch.isfinite(dout).all())
    return o, dqkv, dtable


def _ref_attn(qkv, table, dout, H, W, heads, ws, shift, scale, dtype, masked=True):
    qkv, table = (t.to(dtype).detach().requires_grad_(True) for t in (qkv, table))
    o = st.window_attention(qkv, table, H, W, heads, ws, shift, scale, masked=masked)
    o.backward(dout.to(dtype))
    return o.detach(), qkv.grad, table.grad


@pytest.mark.parametrize("B,H,W,C,heads,ws,shift", ATTN_CASES)
def test_window_attention_against_float64(B, H, W, C, heads, ws, shift):
    qkv, table, scale = _attn_inputs(B, H, W, C, heads, ws)
    dout = torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(ws + 17)).cuda()
    what = f"window attention {B} x {H} x {W}, {heads} heads of {C // heads}, window {ws}, shift {shift}"
    got = _lib_attn(qkv, table, dout, H, W, heads, ws, shift, scale)
    r64 = _ref_attn(qkv, table, dout, H, W, heads, ws, shift, scale, torch.float64)
    r32 = _ref_attn(qkv, table, dout, H, W, heads, ws, shift, scale, torch.float32)
    if ws == 1:
        # one token per window: P = 1 and dS = 0 exactly, in fp32 as in float64.  The yardstick is exact, so the engine must be too.
        o, dqkv, dtable = got
        assert torch.equal(o, qkv[:, :, 2 * C:]) and torch.equal(dqkv[:, :, 2 * C:], dout)
        assert torch.all(dqkv[:, :, :2 * C] == 0) and torch.all(dtable == 0)
        assert torch.equal(dqkv.double(), r64[1]) and torch.equal(dtable.double(), r64[2])
    else:
        rms = [_bar(g, y32, y64, f"{what}: {n}") for n, g, y32, y64 in zip(("out", "dqkv", "dtable"), got, r32, r64)]
        if shift:
            # the test can see the mask: without it the float64 gradient is far away
            free = _ref_attn(qkv, table, dout, H, W, heads, ws, shift, scale, torch.float64, masked=False)
            d = float((free[1] - r64[1]).pow(2).mean().sqrt())
            print(f"{what}: the unmasked dqkv is {d:.3e} rms away")
            assert d > 1000 * rms[1], (what, d, rms[1])
    assert all(torch.equal(p, q) for p, q in zip(got, _lib_attn(qkv, table, dout, H, W, heads, ws, shift, scale)))      # two runs
    for i in range(B if B > 1 else 0):
        o1, d1, _ = _lib_attn(qkv[i:i + 1].contiguous(), table, dout[i:i + 1].contiguous(), H, W, heads, ws, shift, scale)
        assert torch.equal(o1[0], got[0][i]) and torch.equal(d1[0], got[1][i]), i


def test_window_attention_keeps_a_nan_in_its_image():
    B, H, W, C, heads, ws, shift = 2, 16, 24, 16, 2, 8, 3
    qkv, table, scale = _attn_inputs(B, H, W, C, heads, ws)
    dout = torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(3)).cuda()
    _, clean, _ = _lib_attn(qkv, table, dout, H, W, heads, ws, shift, scale)
    bad = dout.clone()
    bad[1, 100, 5] = float("nan")
    _, dirty, _ = _lib_attn(qkv, table, bad, H, W, heads, ws, shift, scale)
    assert torch.equal(dirty[0], clean[0]) and not torch.isfinite(dirty[1]).all()


# ---------------------------------------------------------------------------------------------------------------
# ops.py: the autograd Functions are the library calls, and in eval the engine's stand-alone kernels
# ---------------------------------------------------------------------------------------------------------------
def _leaf(*ts):
    return [t.detach().clone().requires_grad_(True) if t is not None else None for t in ts]


def test_ops_autograd_is_the_library_bit_for_bit():
    from xmm_superres_denoise import ops
    a, w, b, dy = _lin_inputs(480, 36, 70, True)
    al, wl, bl = _leaf(a, w, b)
    y = ops.linear(al.view(2, 240, 36), wl, bl, act="gelu", chunk=112)
    y.backward(dy.view(2, 240, 70))
    ref = _lib_gemm(a, w, b, "gelu", dy, 112)
    assert all(torch.equal(p.reshape(q.shape), q) for p, q in zip((y, al.grad, wl.grad, bl.grad), ref))
    x, w, b, dy = _conv_inputs(2, 5, 7, 6, 6)
    xl, wl, bl = _leaf(x, w, b)
    y = ops.conv3x3(xl, wl, bl, act="lrelu")
    y.backward(dy)
    assert all(torch.equal(p, q) for p, q in zip((y, xl.grad, wl.grad, bl.grad), _lib_gemm(x, w, b, "lrelu", dy, 0, True)))
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(2, 37, 65, generator=g).cuda(), torch.randn(2, 37, 65, generator=g).cuda()
    w, b = _ln_params(65, g)
    xl, wl, bl = _leaf(x, w, b)
    y = ops.layer_norm(xl, wl, bl)
    y.backward(dy)
    ref = _lib_ln(x.view(-1, 65), w, b, dy.view(-1, 65))
    assert all(torch.equal(p.reshape(q.shape), q) for p, q in zip((y, xl.grad, wl.grad, bl.grad), ref))
    B, H, W, C, heads, ws, shift = 2, 9, 18, 10, 2, 9, 4
    qkv, table, scale = _attn_inputs(B, H, W, C, heads, ws)
    dout = torch.randn(B, H * W, C, generator=g).cuda()
    ql, tl = _leaf(qkv, table)
    o = ops.window_attention(ql, tl, H, W, heads, ws, shift, scale)
    o.backward(dout)
    assert all(torch.equal(p, q) for p, q in zip((o, ql.grad, tl.grad), _lib_attn(qkv, table, dout, H, W, heads, ws, shift, scale)))
    # only the gradients that are asked for
    xl, = _leaf(x)
    ops.layer_norm(xl, w, b).backward(dy)
    assert torch.equal(xl.grad.view(-1, 65), ref[1]) and w.grad is None


@pytest.mark.parametrize("grad", [False, True])
def test_ops_forward_is_the_engines_kernel_bit_for_bit(grad):
    """layer_norm, window_attention: the same kernel with the same arguments as engine.sw_*.  linear and conv3x3 are a kernel of their own
    (double sums, one rounding; held to float64 above): within a few ulp of engine.sw_gemm / sw_conv3x3, and the same bits with and without
    a gradient, where the activation runs as a second kernel on the stored pre-activation by the epilogue's own expression."""
    from xmm_superres_denoise import engine, ops
    a, w, b, _ = _lin_inputs(480, 36, 70, True)
    x, cw, cb, _ = _conv_inputs(2, 5, 7, 6, 6)
    g = torch.Generator().manual_seed(11)
    lx = torch.randn(37, 65, generator=g).cuda()
    lw, lb = _ln_params(65, g)
    qkv, table, scale = _attn_inputs(2, 9, 18, 10, 2, 9)
    if grad:
        a, w, b, x, cw, cb, lx, lw, lb, qkv, table = _leaf(a, w, b, x, cw, cb, lx, lw, lb, qkv, table)
    with torch.set_grad_enabled(grad):
        for act in (None, "gelu", "lrelu"):
            y = ops.linear(a, w, b, act=act)
            with torch.no_grad():
                assert y.requires_grad == grad and torch.equal(y, ops.linear(a, w, b, act=act))
            assert (y - engine.sw_gemm(a.detach(), w.detach(), b.detach(), act=act)).abs().max() <= 4 * 2.0 ** -24 * y.abs().max()
            y = ops.conv3x3(x, cw, cb, act=act)
            with torch.no_grad():
                assert y.requires_grad == grad and torch.equal(y, ops.conv3x3(x, cw, cb, act=act))
            assert (y - engine.sw_conv3x3(x.detach(), cw.detach(), cb.detach(), act=act)).abs().max() <= 4 * 2.0 ** -24 * y.abs().max()
        assert torch.equal(ops.layer_norm(lx, lw, lb), engine.sw_layernorm(lx.detach(), lw.detach(), lb.detach()))
        o = ops.window_attention(qkv, table, 9, 18, 2, 9, 4, scale)
        assert torch.equal(o, engine.sw_window_attention(qkv.detach(), table.detach(), 9, 18, 2, 9, 4, scale))


def test_ops_save_nothing_without_a_gradient_and_refuse_a_second_differentiation():
    from xmm_superres_denoise import ops
    a, w, b, dy = _lin_inputs(7, 10, 12, True)
    wl, = _leaf(w)
    for ctx in (torch.no_grad(), torch.inference_mode()):
        with ctx:
            y = ops.linear(a, wl, b, act="gelu")
        assert y.grad_fn is None and not y.requires_grad
    al, = _leaf(a)
    y = ops.linear(al, wl, b, act="gelu")
    g, = torch.autograd.grad(y, al, dy.requires_grad_(True), create_graph=True)        # a gradient of the gradient is asked for
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched for a refused call
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_from_python():
    from xmm_superres_denoise import ops
    from xmm_superres_denoise.engine import XsdError
    z = lambda *s: torch.zeros(*s, device="cuda")         # noqa: E731
    with pytest.raises(XsdError, match="math mode 'bf16x6' is not supported by the differentiable ops"):
        ops.linear(z(4, 8), z(6, 8), math="bf16x6")
    with pytest.raises(XsdError, match="math mode 'bf16x6' is not supported by the differentiable ops"):
        ops.conv3x3(z(1, 4, 4, 2), z(6, 2, 3, 3), math="bf16x6")
    with pytest.raises(XsdError, match="unknown math mode 'f16x3'"):
        ops.linear(z(4, 8), z(6, 8), math="f16x3")
    with pytest.raises(XsdError, match="unknown activation 'relu'"):
        ops.linear(z(4, 8), z(6, 8), act="relu")
    with pytest.raises(XsdError, match=r"are not \[\.\.\., K\] and \[N, K\]"):
        ops.linear(z(4, 8), z(6, 9))
    with pytest.raises(XsdError, match="bias has 5 elements for 6 outputs"):
        ops.linear(z(4, 8), z(6, 8), z(5))
    with pytest.raises(XsdError, match="a must be contiguous"):
        ops.linear(z(8, 4).t(), z(6, 8))
    with pytest.raises(XsdError, match="no CPU fallback"):
        ops.linear(torch.zeros(4, 8), z(6, 8))
    with pytest.raises(XsdError, match="must be float32"):
        ops.layer_norm(z(4, 8).double(), z(8), z(8))
    with pytest.raises(XsdError, match=r"are not \[B, H, W, cin\] and \[N, cin, 3, 3\]"):
        ops.conv3x3(z(1, 4, 4, 2), z(6, 3, 3, 3))
    with pytest.raises(XsdError, match=r"4097 channels are outside \[1, 4096\]"):
        ops.layer_norm(z(2, 4097), z(4097), z(4097))
    with pytest.raises(XsdError, match=r"are not \[\.\.\., C\], \[C\] and \[C\]"):
        ops.layer_norm(z(2, 8), z(7), z(8))
    for kw, msg in ((dict(ws=17, H=17, W=17), r"window size 17 is outside \[1, 16\]"), (dict(H=10), "multiples of the window size 4; got 10 x 8"),
                    (dict(shift=4), r"shift 4 is outside \[0, window size 4\)"), (dict(C=66), "head dim 33; the kernel takes at most 32"),
                    (dict(C=9), "2 heads do not divide 9 channels")):
        c = dict(B=1, H=8, W=8, C=8, heads=2, ws=4, shift=0)
        c.update(kw)
        with pytest.raises(XsdError, match=msg):
            ops.window_attention(z(c["B"], c["H"] * c["W"], 3 * c["C"]), z((2 * c["ws"] - 1) ** 2, c["heads"]), c["H"], c["W"], c["heads"], c["ws"],
                                 c["shift"], 1.0)
    with pytest.raises(XsdError, match="do not fit 8 x 8, 2 heads, window 4"):
        ops.window_attention(z(1, 64, 24), z(49, 3), 8, 8, 2, 4, 0, 1.0)


def test_refusals_of_the_library_itself():
    """what the wrappers cannot express goes through the C entries; the pointers are valid and nothing is launched"""
    L, t = _lib(), torch.zeros(4096, device="cuda")
    p, n = t.data_ptr(), 4 * t.numel()
    err = lambda: L.xsd_last_error().decode()             # noqa: E731
    # linear: (a, w, bias, y, z, M, K, N, act, slope, math, scratch, bytes, stream)
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 4, 8, 6, 0, 0.01, 3, p, n, None) != 0
    assert "linear: math mode bf16x6 is not supported by the differentiable ops" in err()
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 4, 8, 6, 0, 0.01, 4, p, n, None) != 0 and "unknown math mode 4" in err()
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 0, 8, 6, 0, 0.01, 0, p, n, None) != 0 and "0 rows are outside [1, 2^28]" in err()
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 4, 0, 6, 0, 0.01, 0, p, n, None) != 0 and "0 inputs and 6 outputs are outside" in err()
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 4, 8, 6, 7, 0.01, 0, p, n, None) != 0 and "activation 7" in err()
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 4, 8, 6, 0, 0.01, 0, p, 16, None) != 0 and "scratch of 16 bytes; 256 are needed" in err()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, p, None)):
        assert L.xsd_sw_op_linear_forward(*args, None, 4, 8, 6, 0, 0.01, 0, p, n, None) != 0 and "linear: null argument" in err()
    assert L.xsd_sw_op_linear_forward(p, p, p, p, None, 4, 8, 6, 0, 0.01, 0, None, n, None) != 0 and "linear: null argument" in err()
    # backward: (dy, a, w, z, da, dw, db, M, K, N, act, slope, math, chunk, scratch, bytes, stream)
    assert L.xsd_sw_op_linear_backward(p, p, p, None, p, p, p, 4, 8, 6, 1, 0.01, 0, 0, p, n, None) != 0 and "linear: null argument" in err()
    assert L.xsd_sw_op_linear_backward(p, p, p, p, p, p, p, 4, 8, 6, 0, 0.01, 3, 0, p, n, None) != 0 and "bf16x6 is not supported" in err()
    assert L.xsd_sw_op_linear_backward(p, p, p, p, p, p, p, 4, 8, 6, 0, 0.01, 0, -1, p, n, None) != 0 and "chunk of -1 rows is negative" in err()
    assert L.xsd_sw_op_linear_backward(p, p, p, p, p, p, p, 5000, 8, 6, 0, 0.01, 0, 1, p, n, None) != 0 and "into 5000 partials; at most 4096" in err()
    assert L.xsd_sw_op_linear_backward(p, p, p, p, p, p, p, 4, 8, 6, 0, 0.01, 0, 0, p, 16, None) != 0 and "scratch of 16 bytes" in err()
    assert L.xsd_sw_op_linear_scratch(0, 8, 6, 0, 0, 1) == -1 and "0 rows are outside" in err()
    # conv3x3: (x, w, bias, y, z, B, H, W, cin, N, act, slope, math, scratch, bytes, stream)
    assert L.xsd_sw_op_conv3x3_forward(p, p, p, p, None, 1, 0, 4, 2, 6, 0, 0.01, 0, p, n, None) != 0 and "1 images of 0 x 4 pixels are outside" in err()
    assert L.xsd_sw_op_conv3x3_forward(p, p, p, p, None, 1, 20000, 20000, 2, 6, 0, 0.01, 0, p, n, None) != 0 and "pixels are outside [1, 2^28] rows" in err()
    assert L.xsd_sw_op_conv3x3_forward(p, p, p, p, None, 1, 4, 4, 2, 6, 0, 0.01, 3, p, n, None) != 0 and "conv3x3: math mode bf16x6" in err()
    assert L.xsd_sw_op_conv3x3_backward(p, p, p, None, p, p, p, 1, 4, 4, 2, 6, 2, 0.01, 0, 0, p, n, None) != 0 and "conv3x3: null argument" in err()
    assert L.xsd_sw_op_conv3x3_backward(p, p, p, p, p, p, p, 1, 4, 4, 2, 6, 0, 0.01, 0, 0, p, 16, None) != 0 and "scratch of 16 bytes" in err()
    assert L.xsd_sw_op_conv3x3_scratch(1, 4, 4, 0, 6, 0, 0, 0) == -1 and "0 inputs and 6 outputs" in err()
    # layer_norm
    for M in (0, (1 << 31) + 1):
        assert L.xsd_sw_op_layernorm_forward(p, p, p, p, M, 8, None) != 0 and f"layer_norm: {M} rows are outside [1, 2^31]" in err()
    assert L.xsd_sw_op_layernorm_backward(p, p, p, p, p, p, 4, 0, p, n, None) != 0 and "layer_norm: 0 channels are outside [1, 4096]" in err()
    assert L.xsd_sw_op_layernorm_backward(p, p, p, p, p, None, 4, 8, p, n, None) != 0 and "weight and bias come together" in err()
    assert L.xsd_sw_op_layernorm_backward(None, p, p, p, p, p, 4, 8, p, n, None) != 0 and "layer_norm: null argument" in err()
    assert L.xsd_sw_op_layernorm_backward(p, p, p, p, p, p, 4, 8, p, 16, None) != 0 and "layer_norm: scratch of 16 bytes" in err()
    assert L.xsd_sw_op_layernorm_backward(p, p, p, p, p, p, 65536 * 128, 8, p, 1 << 40, None) != 0 and "too many for the weight gradient" in err()
    assert L.xsd_sw_op_layernorm_scratch(4, 4097) == -1 and "4097 channels" in err()
    # window_attention: forward (qkv, table, out, B, H, W, C, heads, ws, shift, scale, stream)
    for B, H, W in ((0, 8, 8), (1, 0, 8), (-1, 8, 8)):
        assert L.xsd_sw_op_attention_forward(p, p, p, B, H, W, 8, 2, 4, 0, 1.0, None) != 0 and f"window_attention: bad shape {B}x{H}x{W}" in err()
    assert L.xsd_sw_op_attention_forward(p, p, p, 1, 16400, 16400, 8, 2, 16, 0, 1.0, None) != 0 and "tokens are too many" in err()
    assert L.xsd_sw_op_attention_forward(p, p, p, 1, 8, 8, 8, 0, 4, 0, 1.0, None) != 0 and "0 heads do not divide 8 channels" in err()
    assert L.xsd_sw_op_attention_forward(p, None, p, 1, 8, 8, 8, 2, 4, 0, 1.0, None) != 0 and "window_attention: null argument" in err()
    # backward (dout, qkv, table, dqkv, dtable, B, H, W, C, heads, ws, shift, scale, scratch, bytes, stream)
    assert L.xsd_sw_op_attention_backward(p, p, p, p, p, 1, 17, 17, 8, 2, 17, 0, 1.0, p, n, None) != 0 and "window size 17 is outside [1, 16]" in err()
    assert L.xsd_sw_op_attention_backward(p, p, p, p, p, 1, 8, 8, 66, 2, 4, 0, 1.0, p, n, None) != 0 and "head dim 33" in err()
    assert L.xsd_sw_op_attention_backward(p, p, p, p, p, 1, 8, 8, 8, 2, 4, 4, 1.0, p, n, None) != 0 and "shift 4 is outside" in err()
    assert L.xsd_sw_op_attention_backward(p, p, p, p, None, 1, 8, 8, 8, 2, 4, 0, 1.0, p, n, None) != 0 and "window_attention: null argument" in err()
    assert L.xsd_sw_op_attention_backward(p, p, p, p, p, 1, 8, 8, 8, 2, 4, 0, 1.0, p, 16, None) != 0 and "scratch of 16 bytes; 1792 are needed" in err()
    assert L.xsd_sw_op_attention_scratch(1, 8, 6, 8, 2, 4) == -1 and "multiples of the window size 4; got 8 x 6" in err()
    torch.cuda.synchronize()
    assert torch.all(t == 0)
