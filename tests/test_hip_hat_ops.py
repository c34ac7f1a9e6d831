"""The differentiable HAT ops (include/xsd.h "differentiable HAT ops", csrc/hat_ops.hip, xmm_superres_denoise/ops.py): overlap_attention
and channel_attention, forward and backward, each against torch's autograd of the plain float64 restatement tests/golden/hat_torch.py
(ocab_attention, channel_attention).  The yardstick is the project's (test_hip_sw_kernels._assert_within_2x_of_fp32): for every compared
tensor the engine's error against float64 is at most twice that of the same restatement in fp32 through torch autograd on the same
device, in rms and in max |err| relative to the tensor's max, and the yardstick's own error must be non-zero.

The library entries are called directly with NaN-filled outputs and sentinel guards behind them (every call of _lib_ocab / _lib_ca
asserts that every element was written and nothing behind it); the autograd Functions of ops.py are then held bit for bit to those
calls, and the forwards to engine.hat_ocab_attention / hat_ca_combine."""
import ctypes

import numpy as np
import pytest
import torch

import gen_hat as gh
import hat_torch as ht
from test_hip_sw_kernels import _assert_within_2x_of_fp32, _guarded, _untouched

pytestmark = pytest.mark.gpu


def _bar(y, y32, y64, what):
    rms32 = _assert_within_2x_of_fp32(y, y32, y64, what)
    assert rms32 > 0, (what, "the fp32 yardstick is exact here: a bar of 0 proves nothing")
    return rms32


def _lib():
    from xmm_superres_denoise.engine import _lib
    return _lib.load()


def _scratch(nbytes):
    assert nbytes >= 0, _lib().xsd_last_error()
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _leaf(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


# ---------------------------------------------------------------------------------------------------------------
# overlap_attention
# ---------------------------------------------------------------------------------------------------------------
#             ws  ow heads hd  B   H   W
OCAB_CASES = {"a border and interior windows": (4, 6, 2, 6, 2, 8, 12),        # every token a key of 1, 2 or 4 windows
              "b no overlap": (4, 4, 1, 5, 1, 4, 8),                          # no padding either
              "c one window": (8, 12, 3, 4, 1, 8, 8),                         # every neighbour is padding
              "d the XMM window": (16, 24, 2, 30, 1, 32, 48),                 # 576 keys, 9 chunks of 64, head dim 30
              "e both limits": (16, 32, 1, 32, 1, 16, 32)}                    # 1024 keys, head dim 32


def _ocab_inputs(ws, ow, heads, hd, B, H, W, seed=0):
    g = torch.Generator().manual_seed(100000 * ws + 1000 * ow + 10 * H + W + seed)
    C = heads * hd
    qkv = torch.randn(B, H * W, 3 * C, generator=g).cuda()
    table = (torch.rand((ws + ow - 1) ** 2, heads, generator=g) - 0.5).cuda()
    dout = torch.randn(B, H * W, C, generator=g).cuda()
    return qkv, table, dout, hd ** -0.5


def _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale):
    """-> out, dqkv, dtable of the library's forward + backward entries on the current stream; every output NaN-filled, guards behind"""
    L = _lib()
    B, _, C3 = (int(v) for v in qkv.shape)
    C = C3 // 3
    outs = [_guarded((B, H * W, C)), _guarded((B, H * W, C3)), _guarded(tuple(table.shape))]
    (o, _), (dqkv, _), (dtable, _) = outs
    assert L.xsd_hat_op_ocab_forward(qkv.data_ptr(), table.data_ptr(), o.data_ptr(), B, H, W, C, heads, ws, ow, scale, _stream()) == 0, \
        L.xsd_last_error()
    s = _scratch(L.xsd_hat_op_ocab_scratch(B, H, W, C, heads, ws, ow))
    s.fill_(0xFF)                                             # a slab or partial that is read without being written is a NaN
    rc = L.xsd_hat_op_ocab_backward(dout.data_ptr(), qkv.data_ptr(), table.data_ptr(), o.data_ptr(), dqkv.data_ptr(), dtable.data_ptr(), B, H, W,
                                    C, heads, ws, ow, scale, s.data_ptr(), s.numel(), _stream())
    assert rc == 0, L.xsd_last_error()
    torch.cuda.current_stream().synchronize()
    for t, g in outs:
        assert _untouched(g) and torch.isfinite(t).all()
    return o, dqkv, dtable


def _ref_ocab(qkv, table, dout, H, W, heads, ws, ow, scale, dtype):
    qkv, table = (t.to(dtype).detach().requires_grad_(True) for t in (qkv, table))
    o = ht.ocab_attention(qkv, table, H, W, heads, ws, ow, scale)
    o.backward(dout.to(dtype))
    return o.detach(), qkv.grad, table.grad


@pytest.mark.parametrize("name", list(OCAB_CASES))
def test_overlap_attention_against_float64(name):
    ws, ow, heads, hd, B, H, W = OCAB_CASES[name]
    C = heads * hd
    qkv, table, dout, scale = _ocab_inputs(*OCAB_CASES[name])
    what = f"overlap attention {name}: {B} x {H} x {W}, {heads} heads of {hd}, window {ws} / {ow}"
    o, dqkv, dtable = got = _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale)
    o64, d64, t64 = _ref_ocab(qkv, table, dout, H, W, heads, ws, ow, scale, torch.float64)
    o32, d32, t32 = _ref_ocab(qkv, table, dout, H, W, heads, ws, ow, scale, torch.float32)
    failed = []
    for n, y, y32, y64 in [("out", o, o32, o64), ("dtable", dtable, t32, t64)] + \
            [(n, dqkv[..., k * C:(k + 1) * C], d32[..., k * C:(k + 1) * C], d64[..., k * C:(k + 1) * C]) for k, n in enumerate(("dq", "dk", "dv"))]:
        try:
            _bar(y, y32, y64, f"{what}: {n}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    assert all(torch.equal(p, q) for p, q in zip(got, _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale)))      # two runs: bit for bit
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale)
    assert all(torch.equal(p, q) for p, q in zip(got, other))                                                        # a side stream: the same bits


@pytest.mark.parametrize("grad", [False, True])
def test_overlap_attention_forward_is_the_engines_kernel_and_autograd_is_the_library(grad):
    from xmm_superres_denoise import engine, ops
    ws, ow, heads, hd, B, H, W = OCAB_CASES["a border and interior windows"]
    qkv, table, dout, scale = _ocab_inputs(ws, ow, heads, hd, B, H, W)
    want = engine.hat_ocab_attention(qkv, table, H, W, heads, ws, ow, scale)
    ql, tl = _leaf(qkv, table) if grad else (qkv, table)
    with torch.set_grad_enabled(grad):
        o = ops.overlap_attention(ql, tl, H, W, heads, ws, ow, scale)
    assert torch.equal(o, want) and o.requires_grad == grad
    for ctx in (torch.no_grad(), torch.inference_mode()):
        with ctx:
            y = ops.overlap_attention(ql, tl, H, W, heads, ws, ow, scale)
        assert y.grad_fn is None and not y.requires_grad and torch.equal(y, want)
    if grad:
        o.backward(dout)
        ref = _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale)
        assert all(torch.equal(p, q) for p, q in zip((o, ql.grad, tl.grad), ref))
        o = ops.overlap_attention(ql, tl, H, W, heads, ws, ow, scale)
        g, = torch.autograd.grad(o, ql, dout.requires_grad_(True), create_graph=True)          # a gradient of the gradient is asked for
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.sum().backward()


def test_overlap_attention_gradient_of_one_window_stays_in_its_patch():
    """dout is non-zero in one window only: dq is zero outside the window, dk / dv are exactly zero at tokens outside that window's
    ow x ow patch and non-zero at every token inside it, the neighbouring windows' tokens included"""
    ws, ow, heads, hd, B, H, W = OCAB_CASES["a border and interior windows"]
    C, pad = heads * hd, (ow - ws) // 2
    qkv, table, dout, scale = _ocab_inputs(ws, ow, heads, hd, B, H, W)
    only = torch.zeros_like(dout).view(B, H, W, C)
    only[0, 0:4, 4:8] = dout.view(B, H, W, C)[0, 0:4, 4:8]                                      # window (0, 1) of image 0
    _, dqkv, _ = _lib_ocab(qkv, table, only.view(B, H * W, C), H, W, heads, ws, ow, scale)
    d = dqkv.view(B, H, W, 3, C)
    inside = torch.zeros(B, H, W, dtype=torch.bool, device="cuda")
    inside[0, 0:4 + pad, 4 - pad:8 + pad] = True                                                # rows -1 .. 4 clipped to 0 .. 4, columns 3 .. 8
    window = torch.zeros_like(inside)
    window[0, 0:4, 4:8] = True
    assert int(inside.sum()) == 5 * 6 and torch.all(d[~window][:, 0] == 0) and torch.all(d[window][:, 0] != 0)
    for k in (1, 2):
        assert torch.all(d[~inside][:, k] == 0), k
        assert torch.all(d[inside][:, k] != 0), k


def test_overlap_attention_table_gradient_bins_against_numpy():
    """q = k = 0 and a table of zeros: every probability is 1 / ow^2, the padded keys' included, so dS = (dP - mean_j dP) / ow^2 with dP = dout . v depends on
    the index arithmetic alone: the table gradient is dS scattered to gen_hat.rel_index_oca, whose negative entries wrap.  (With v = 0 as
    well the output does not depend on the table and the gradient is identically 0: v stays.)  numpy in float64 is the reference, the same
    numpy in float32 the yardstick."""
    ws, ow, heads, hd, B, H, W = 4, 6, 2, 6, 1, 8, 12
    C, pad, NK = heads * hd, 1, 36
    qkv, table, dout, scale = _ocab_inputs(ws, ow, heads, hd, B, H, W, seed=7)
    qkv[..., :2 * C] = 0
    table.zero_()
    idx = gh.rel_index_oca(ws, ow)
    assert idx.min() < 0 and idx.max() < (ws + ow - 1) ** 2
    _, _, dtable = _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale)

    def numpy_dtable(dtype):
        v = np.zeros((H + 2 * pad, W + 2 * pad, C), dtype)
        v[pad:-pad, pad:-pad] = qkv[0, :, 2 * C:].cpu().numpy().reshape(H, W, C).astype(dtype)
        g = dout[0].cpu().numpy().reshape(H, W, C).astype(dtype)
        dt = np.zeros(((ws + ow - 1) ** 2, heads), dtype)
        for wy in range(H // ws):
            for wx in range(W // ws):
                for h in range(heads):
                    vp = v[wy * ws:wy * ws + ow, wx * ws:wx * ws + ow, h * hd:(h + 1) * hd].reshape(NK, hd)
                    gw = g[wy * ws:(wy + 1) * ws, wx * ws:(wx + 1) * ws, h * hd:(h + 1) * hd].reshape(ws * ws, hd)
                    dp = gw @ vp.T
                    np.add.at(dt[:, h], idx, ((dp - dp.mean(1, keepdims=True)) / dtype(NK)).astype(dtype))
        return dt
    d64 = numpy_dtable(np.float64)
    assert np.count_nonzero(d64[idx.min():]) > 0                                                 # the wrapped bins carry a gradient
    _bar(dtable, numpy_dtable(np.float32), d64, "overlap attention, q = k = 0: dtable against numpy over rel_index_oca")
    _, _, t64 = _ref_ocab(qkv, table, dout, H, W, heads, ws, ow, scale, torch.float64)
    assert np.abs(t64.cpu().numpy() - d64).max() <= 1e-12 * np.abs(d64).max()                    # the two references agree


# ---------------------------------------------------------------------------------------------------------------
# channel_attention
# ---------------------------------------------------------------------------------------------------------------
CA_CASES = [(1, 1, 1, 1), (2, 96, 12, 3), (3, 257, 180, 6), (2, 600, 7, 2)]      # 257: past the pool's chunk of 256; 180 / 6: the XMM widths
CA_SEED = {(1, 1, 1, 1): 1}      # seed 0 draws a hidden unit whose ReLU is off: dw1, db1 and dw2 are then 0 in fp32 too, a yardstick of 0


def _ca_inputs(B, HW, C, Cs, seed=0):
    g = torch.Generator().manual_seed(100000 * B + 100 * HW + C + seed)
    t = (torch.randn(B, HW, C, generator=g) + 0.5 * torch.randn(1, 1, C, generator=g)).cuda()

    def u(*shape, fan):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * 3 / fan ** 0.5).cuda()
    w1, b1, w2, b2 = u(Cs, C, 1, 1, fan=C), u(Cs, fan=C).abs(), u(C, Cs, 1, 1, fan=Cs), u(C, fan=Cs)
    return t, w1, b1, w2, b2, torch.randn(B, HW, C, generator=g).cuda()


def _lib_ca(t, w1, b1, w2, b2, dy):
    """-> y, gates, dt, dw1, db1, dw2, db2 of the library's forward + backward entries on the current stream"""
    L = _lib()
    B, HW, C = (int(v) for v in t.shape)
    Cs = int(b1.numel())
    outs = [_guarded(tuple(t.shape)), _guarded((B, C)), _guarded(tuple(t.shape))] + [_guarded(tuple(v.shape)) for v in (w1, b1, w2, b2)]
    y, gates, dt, dw1, db1, dw2, db2 = (o for o, _ in outs)
    s = _scratch(L.xsd_hat_op_ca_scratch(B, HW, C, Cs, 0))
    s.fill_(0xFF)
    rc = L.xsd_hat_op_ca_forward(t.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), gates.data_ptr(), B, HW, C,
                                 Cs, s.data_ptr(), s.numel(), _stream())
    assert rc == 0, L.xsd_last_error()
    s = _scratch(L.xsd_hat_op_ca_scratch(B, HW, C, Cs, 1))
    s.fill_(0xFF)
    rc = L.xsd_hat_op_ca_backward(dy.data_ptr(), t.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dt.data_ptr(),
                                  dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), B, HW, C, Cs, s.data_ptr(),
                                  s.numel(), _stream())
    assert rc == 0, L.xsd_last_error()
    torch.cuda.current_stream().synchronize()
    for o, g in outs:
        assert _untouched(g) and torch.isfinite(o).all()
    return y, gates, dt, dw1, db1, dw2, db2


def _ref_ca(t, w1, b1, w2, b2, dy, dtype):
    """hat_torch.channel_attention on the [B, C, HW, 1] image of the token-major t -> y, dt (both token-major), dw1, db1, dw2, db2"""
    tl, *ws = (v.to(dtype).detach().requires_grad_(True) for v in (t, w1, b1, w2, b2))
    sd = dict(zip(("attention.1.weight", "attention.1.bias", "attention.3.weight", "attention.3.bias"), ws))
    y = ht.channel_attention(tl.transpose(1, 2).unsqueeze(-1), sd, "").squeeze(-1).transpose(1, 2)
    y.backward(dy.to(dtype))
    return (y.detach(), tl.grad) + tuple(w.grad for w in ws)


@pytest.mark.parametrize("B,HW,C,Cs", CA_CASES)
def test_channel_attention_against_float64(B, HW, C, Cs):
    from xmm_superres_denoise import engine
    t, w1, b1, w2, b2, dy = _ca_inputs(B, HW, C, Cs, seed=CA_SEED.get((B, HW, C, Cs), 0))
    what = f"channel attention {B} x {HW} x {C}, squeezed to {Cs}"
    y, gates, *grads = got = _lib_ca(t, w1, b1, w2, b2, dy)
    want = torch.empty_like(gates)
    engine.hat_ca_combine(torch.zeros_like(t), t, w1, b1, w2, b2, 1.0, gates=want)
    assert torch.equal(gates, want), what                                                       # bitwise the dev_y of xsd_hat_test_ca_combine
    r64, r32 = _ref_ca(t, w1, b1, w2, b2, dy, torch.float64), _ref_ca(t, w1, b1, w2, b2, dy, torch.float32)
    failed = []
    for n, g, y32, y64 in zip(("y", "dt", "dw1", "db1", "dw2", "db2"), [y] + grads, r32, r64):
        try:
            _bar(g, y32, y64, f"{what}: {n}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    assert all(torch.equal(p, q) for p, q in zip(got, _lib_ca(t, w1, b1, w2, b2, dy)))          # two runs: bit for bit
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _lib_ca(t, w1, b1, w2, b2, dy)
    assert all(torch.equal(p, q) for p, q in zip(got, other))                                   # a side stream: the same bits


def test_channel_attention_relu_mask_is_per_image():
    """hidden unit 0 is off for image 0 and on for image 1: its row of dw1 (and its db1) is image 1's alone, to the bit; unit 1 is on
    for both (a large bias)"""
    B, HW, C, Cs = 2, 96, 12, 3
    t, w1, b1, w2, b2, dy = _ca_inputs(B, HW, C, Cs, seed=1)
    w1[0] = w1[0].abs() + 0.1
    b1[0], b1[1] = 0.0, 50.0
    t[0] = -t[0].abs() - 1.0
    t[1] = t[1].abs() + 1.0
    _, _, _, dw1, db1, _, _ = _lib_ca(t, w1, b1, w2, b2, dy)
    _, _, _, off1, offb, _, _ = _lib_ca(t[:1].contiguous(), w1, b1, w2, b2, dy[:1].contiguous())
    _, _, _, on1, onb, _, _ = _lib_ca(t[1:].contiguous(), w1, b1, w2, b2, dy[1:].contiguous())
    assert torch.all(off1[0] == 0) and float(offb[0]) == 0.0 and torch.all(on1[0] != 0) and float(onb[0]) != 0.0
    assert torch.equal(dw1[0], on1[0]) and torch.equal(db1[0], onb[0])
    assert not torch.equal(dw1[1], on1[1])                                                       # a unit that is on in both images sums both


def test_channel_attention_autograd_is_the_library_and_saves_nothing_without_a_gradient():
    from xmm_superres_denoise import ops
    t, w1, b1, w2, b2, dy = _ca_inputs(2, 96, 12, 3)
    ref = _lib_ca(t, w1, b1, w2, b2, dy)
    leaves = _leaf(t, w1, b1, w2, b2)
    y = ops.channel_attention(*leaves)
    y.backward(dy)
    assert torch.equal(y, ref[0]) and all(torch.equal(p.grad, q) for p, q in zip(leaves, ref[2:]))
    y4 = ops.channel_attention(t.view(2, 8, 12, 12), w1, b1, w2, b2)                             # [B, H, W, C] and no gradient asked for
    assert y4.shape == (2, 8, 12, 12) and torch.equal(y4.view(2, 96, 12), ref[0]) and y4.grad_fn is None
    tl, = _leaf(t)
    ops.channel_attention(tl, w1, b1, w2, b2).backward(dy)                                       # only the gradient that is asked for
    assert torch.equal(tl.grad, ref[2]) and w1.grad is None
    for ctx in (torch.no_grad(), torch.inference_mode()):
        with ctx:
            y = ops.channel_attention(*leaves)
        assert y.grad_fn is None and not y.requires_grad and torch.equal(y, ref[0])
    y = ops.channel_attention(*leaves)
    g, = torch.autograd.grad(y, leaves[0], dy.requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---------------------------------------------------------------------------------------------------------------
# both ops
# ---------------------------------------------------------------------------------------------------------------
def test_neither_op_allocates_or_frees_device_memory():
    """xsd_test_mem_stats counts every allocation and free of the library (exact integers): a forward and a backward of each op move
    neither"""
    def moved():
        buf = (ctypes.c_int64 * 6)()
        assert _lib().xsd_test_mem_stats(buf, 6) == 0
        return int(buf[2]), int(buf[3])                                                          # allocs, frees
    ws, ow, heads, hd, B, H, W = OCAB_CASES["a border and interior windows"]
    qkv, table, dout, scale = _ocab_inputs(ws, ow, heads, hd, B, H, W)
    t, w1, b1, w2, b2, dy = _ca_inputs(2, 96, 12, 3)
    torch.cuda.synchronize()
    before = moved()
    _lib_ocab(qkv, table, dout, H, W, heads, ws, ow, scale)
    _lib_ca(t, w1, b1, w2, b2, dy)
    torch.cuda.synchronize()
    assert moved() == before


def test_refusals_of_the_library_itself():
    """the pointers are valid and nothing is launched for a refused call"""
    L, t = _lib(), torch.zeros(1 << 16, device="cuda")
    p, n = t.data_ptr(), 4 * t.numel()
    err = lambda: L.xsd_last_error().decode()             # noqa: E731

    def fwd(B=1, H=8, W=8, C=8, heads=2, ws=4, ow=6, ptrs=(p, p, p)):
        return L.xsd_hat_op_ocab_forward(*ptrs, B, H, W, C, heads, ws, ow, 1.0, None)

    def bwd(B=1, H=8, W=8, C=8, heads=2, ws=4, ow=6, ptrs=(p,) * 6, scratch=p, nbytes=n):
        return L.xsd_hat_op_ocab_backward(*ptrs, B, H, W, C, heads, ws, ow, 1.0, scratch, nbytes, None)
    for call in (fwd, bwd):
        assert call(H=17, W=17, ws=17, ow=19) != 0 and "overlap_attention: window size 17 is outside [1, 16]" in err()
        assert call(H=16, W=16, ws=16, ow=34) != 0 and "overlap_attention: overlap window 34 is outside [window size 16, 32]" in err()
        assert call(ow=7) != 0 and "overlap_attention: overlap window 7 minus window size 4 is odd" in err()
        assert call(C=66) != 0 and "overlap_attention: head dim 33; the kernel takes at most 32" in err()
        assert call(W=10) != 0 and "overlap_attention: H and W must be multiples of the window size 4; got 8 x 10" in err()
        assert call(B=0) != 0 and "overlap_attention: bad shape 0x8x8" in err()
    for i in range(3):
        assert fwd(ptrs=tuple(None if k == i else p for k in range(3))) != 0 and "overlap_attention: null argument" in err()
    for i in range(6):
        assert bwd(ptrs=tuple(None if k == i else p for k in range(6))) != 0 and "overlap_attention: null argument" in err()
    assert bwd(scratch=None) != 0 and "overlap_attention: null argument" in err()
    need = L.xsd_hat_op_ocab_scratch(1, 8, 8, 8, 2, 4, 6)
    assert need == 4 * 4 * 36 * 16 + 4 * 4 * 81 * 2 + (-(4 * 4 * 81 * 2) % 256) and need <= n
    assert bwd(nbytes=need - 1) != 0 and f"overlap_attention: scratch of {need - 1} bytes; {need} are needed" in err()
    # channel_attention: forward (t, w1, b1, w2, b2, y, gates, B, HW, C, Cs, scratch, bytes, stream)
    for i in range(6):                                                                           # the gates may be NULL: kept in scratch
        assert L.xsd_hat_op_ca_forward(*(None if k == i else p for k in range(7)), 1, 4, 8, 2, p, n, None) != 0
        assert "channel_attention: null argument" in err()
    assert L.xsd_hat_op_ca_forward(*(p,) * 7, 1, 4, 8, 2, None, n, None) != 0 and "channel_attention: null argument" in err()
    need = L.xsd_hat_op_ca_scratch(1, 4, 8, 2, 0)
    assert need == 512 and L.xsd_hat_op_ca_forward(*(p,) * 7, 1, 4, 8, 2, p, need - 1, None) != 0
    assert "channel_attention: scratch of 511 bytes; 512 are needed" in err()
    assert L.xsd_hat_op_ca_forward(*(p,) * 7, 1, 4, 4097, 2, p, n, None) != 0 and "channel_attention: 4097 channels are outside [1, 4096]" in err()
    # backward (dy, t, w1, b1, w2, b2, dt, dw1, db1, dw2, db2, B, HW, C, Cs, scratch, bytes, stream)
    for i in range(11):
        assert L.xsd_hat_op_ca_backward(*(None if k == i else p for k in range(11)), 1, 4, 8, 2, p, n, None) != 0
        assert "channel_attention: null argument" in err()
    need = L.xsd_hat_op_ca_scratch(1, 4, 8, 2, 1)
    assert need == 256 + 256 + 8 * (2 * 2 * 8 + 2 + 8) + (-(8 * 42) % 256)                      # 8 x 16, 8 x 26 and 8 x 42 bytes, each rounded up
    assert L.xsd_hat_op_ca_backward(*(p,) * 11, 1, 4, 8, 2, p, need - 1, None) != 0
    assert f"channel_attention: scratch of {need - 1} bytes; {need} are needed" in err()
    assert L.xsd_hat_op_ca_backward(*(p,) * 11, 1, 4, 8, 0, p, n, None) != 0 and "channel_attention: a squeezed width of 0 is outside" in err()
    assert L.xsd_hat_op_ca_backward(*(p,) * 11, 65536, 4, 8, 2, p, n, None) != 0 and "channel_attention: 65536 images are outside" in err()
    torch.cuda.synchronize()
    assert torch.all(t == 0)


def test_refusals_from_python():
    from xmm_superres_denoise import ops
    from xmm_superres_denoise.engine import XsdError
    z = lambda *s: torch.zeros(*s, device="cuda")         # noqa: E731
    for kw, msg in ((dict(ws=17, ow=19, H=17, W=17), r"window size 17 is outside \[1, 16\]"), (dict(ws=16, ow=34, H=16, W=16), "overlap window 34 is outside"),
                    (dict(ow=7), "overlap window 7 minus window size 4 is odd"), (dict(C=66), "head dim 33; the kernel takes at most 32"),
                    (dict(H=10), "multiples of the window size 4; got 10 x 8")):
        c = dict(B=1, H=8, W=8, C=8, heads=2, ws=4, ow=6)
        c.update(kw)
        with pytest.raises(XsdError, match="overlap_attention: .*" + msg):
            ops.overlap_attention(z(c["B"], c["H"] * c["W"], 3 * c["C"]), z((c["ws"] + c["ow"] - 1) ** 2, c["heads"]), c["H"], c["W"], c["heads"],
                                  c["ws"], c["ow"], 1.0)
    with pytest.raises(XsdError, match="do not fit 8 x 8, 2 heads, window 4, overlap window 6"):
        ops.overlap_attention(z(1, 64, 24), z(49, 2), 8, 8, 2, 4, 6, 1.0)
    with pytest.raises(XsdError, match="qkv must be float32"):
        ops.overlap_attention(z(1, 64, 24).double(), z(81, 2), 8, 8, 2, 4, 6, 1.0)
    with pytest.raises(XsdError, match="are not .* a squeeze MLP of 8 channels"):
        ops.channel_attention(z(1, 16, 8), z(2, 7, 1, 1), z(2), z(8, 2, 1, 1), z(8))
    with pytest.raises(XsdError, match="t must be contiguous"):
        ops.channel_attention(z(1, 8, 16).transpose(1, 2), z(2, 8, 1, 1), z(2), z(8, 2, 1, 1), z(8))
    with pytest.raises(XsdError, match=r"channel_attention: 4097 channels are outside \[1, 4096\]"):
        ops.channel_attention(z(1, 2, 4097), z(2, 4097, 1, 1), z(2), z(4097, 2, 1, 1), z(4097))
