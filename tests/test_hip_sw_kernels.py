"""The kernels that SwinFIR and HAT run besides the GEMM, each on its own through its test hook (include/xsd.h) against a plain float64
reference of the same operation: the shifted-window attention (csrc/sw_kernels.h, all eight tile counts, head dims 1 .. 32), the token
LayerNorm, and HAT's channel attention + combine (csrc/hat.hip), across the shapes the constructors accept; then two whole networks at
SwinFIR's published window of 12.  The yardstick is the same reference in fp32 on the same device, the bar the project's 2x.  Every
output buffer is pre-filled (NaN where the kernel must write, a finite sentinel in guard elements behind it)."""
import numpy as np
import pytest
import torch

import gen_hat as gh
import gen_swinfir as gs
import hat_torch as ht
import swinfir_torch as st

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
EPS = 2.0 ** -24


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    scale = np.abs(ref).max()
    return float(np.sqrt((e ** 2).mean())), float(e.max() / scale) if scale > 0 else float(e.max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    y, y32, y64 = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (y, y32, y64))
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)
    return rms32


def _guarded(shape, guard=300):
    """a NaN-filled contiguous tensor of `shape` with `guard` sentinel elements behind it in the same allocation"""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), SENTINEL, device="cuda")
    buf[:n] = float("nan")
    return buf[:n].view(shape), buf[n:]


def _untouched(guard):
    return bool(torch.all(guard == SENTINEL))


# ---------------------------------------------------------------------------------------------------------------
# window attention
# ---------------------------------------------------------------------------------------------------------------
ATTN_CASES = [
    (1, 24, 36, 60, 2, 12, 6),       # 5 tiles, head dim 30, SwinFIR's own window
    (2, 9, 18, 10, 2, 9, 4),         # 3 tiles, odd head dim 5, a single row of shifted windows (H == ws)
    (1, 20, 10, 32, 1, 10, 5),       # 4 tiles, head dim 32: no padded lane
    (1, 14, 28, 6, 6, 14, 7),        # 7 tiles, head dim 1
    (1, 30, 15, 24, 3, 15, 0),       # 8 tiles with 225 of 256 tokens
    (1, 11, 22, 16, 2, 11, 5),       # 4 tiles
    (2, 16, 32, 180, 6, 16, 8),      # the XMM block
    (1, 6, 9, 8, 2, 3, 1),
    (1, 16, 24, 16, 2, 8, 3),        # a shift that is not ws / 2
    (1, 2, 3, 4, 2, 1, 0),           # one token per window: the output is v
    (1, 13, 26, 12, 2, 13, 6),       # 6 tiles: with the above, every instantiation 1 .. 8
]


def _attn_inputs(B, H, W, C, heads, ws):
    g = torch.Generator().manual_seed(100000 * ws + 1000 * H + W)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).cuda()
    table = (torch.rand((2 * ws - 1) ** 2, heads, generator=g) - 0.5).cuda()
    return qkv, table, (C // heads) ** -0.5


def test_attention_cases_launch_every_instantiation():
    assert {(ws * ws + 31) // 32 for *_, ws, _ in ATTN_CASES} == set(range(1, 9))


@pytest.mark.parametrize("B,H,W,C,heads,ws,shift", ATTN_CASES)
def test_window_attention_against_float64(B, H, W, C, heads, ws, shift):
    from xmm_superres_denoise.engine import sw_window_attention
    qkv, table, scale = _attn_inputs(B, H, W, C, heads, ws)
    what = f"window attention {B} x {H} x {W}, {heads} heads of {C // heads}, window {ws}, shift {shift}"
    out, guard = _guarded((B, H * W, C))
    o = sw_window_attention(qkv, table, H, W, heads, ws, shift, scale, out=out)
    assert o.data_ptr() == out.data_ptr() and torch.isfinite(o).all() and _untouched(guard), what
    o64 = st.window_attention(qkv.double(), table.double(), H, W, heads, ws, shift, scale)
    o32 = st.window_attention(qkv, table, H, W, heads, ws, shift, scale)
    rms32 = _assert_within_2x_of_fp32(o, o32, o64, what)
    if shift:
        # the test can see the mask: without it the reference is far away
        free = st.window_attention(qkv.double(), table.double(), H, W, heads, ws, shift, scale, masked=False)
        d = float((free - o64).pow(2).mean().sqrt())
        print(f"{what}: the unmasked reference is {d:.3e} rms away")
        assert d > 1000 * rms32, (what, d, rms32)
    if ws == 1:
        assert torch.equal(o, qkv[:, :, 2 * C:])                     # softmax over one key is 1
    assert torch.equal(sw_window_attention(qkv, table, H, W, heads, ws, shift, scale), o)      # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        assert torch.equal(sw_window_attention(qkv[i:i + 1].contiguous(), table, H, W, heads, ws, shift, scale)[0], o[i]), i


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
def _ln_check(x, w, b, what, guard_rows=3):
    from xmm_superres_denoise.engine import sw_layernorm
    M, C = x.shape
    buf = torch.full((M + guard_rows, C), SENTINEL, device="cuda")
    buf[:M] = float("nan")
    y = sw_layernorm(x, w, b, out=buf)[:M]
    assert torch.isfinite(y).all() and _untouched(buf[M:]), what
    y64 = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), eps=1e-5)
    y32 = torch.nn.functional.layer_norm(x, (C,), w, b, eps=1e-5)
    _assert_within_2x_of_fp32(y, y32, y64, what)
    assert torch.equal(sw_layernorm(x, w, b), y)                     # two runs: bit for bit
    k = min(M, 5)
    assert torch.equal(sw_layernorm(x[M - k:].contiguous(), w, b), y[M - k:])      # a row does not depend on the rows beside it


def _ln_params(C, g):
    return (1 + 0.4 * (torch.rand(C, generator=g) - 0.5)).cuda(), (0.4 * (torch.rand(C, generator=g) - 0.5)).cuda()


@pytest.mark.parametrize("M,C", [(5, 180), (4, 64), (7, 65), (3, 2), (1030, 24), (9, 4096)])
def test_layernorm_against_float64(M, C):
    g = torch.Generator().manual_seed(1000 * M + C)
    x = (torch.randn(M, C, generator=g) * 3 + 0.7).cuda()
    w, b = _ln_params(C, g)
    _ln_check(x, w, b, f"LayerNorm {M} x {C}")


def test_layernorm_of_a_large_mean_with_a_small_spread():
    """rows of 1000 + 1e-3 randn: one ulp of the values is 6e-5 of a spread of 1e-3, so the statistics have to be carried in double"""
    g = torch.Generator().manual_seed(77)
    x = (1000 + 1e-3 * torch.randn(64, 180, generator=g)).cuda()
    w, b = _ln_params(180, g)
    _ln_check(x, w, b, "LayerNorm 64 x 180, 1000 + 1e-3 randn")


# ---------------------------------------------------------------------------------------------------------------
# HAT: channel attention + combine
# ---------------------------------------------------------------------------------------------------------------
def _ca_inputs(B, HW, C, Cs):
    g = torch.Generator().manual_seed(100000 * B + 100 * HW + C)
    x = torch.randn(B, HW, C, generator=g).cuda()
    t = (torch.randn(B, HW, C, generator=g) + 0.5 * torch.randn(1, 1, C, generator=g)).cuda()

    def u(*shape, fan):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * 3 / fan ** 0.5).cuda()
    return x, t, u(Cs, C, fan=C), u(Cs, fan=C), u(C, Cs, fan=Cs), u(C, fan=Cs)


def _ca_reference(x, t, w1, b1, w2, b2, scale):
    y = torch.sigmoid(torch.relu(t.mean(1) @ w1.T + b1) @ w2.T + b2)
    return x + (t * y[:, None, :]) * scale, y


def _gate_bound(t, w1, b1, w2, b2):
    """what the fp32 roundings of hat_ca_kernel can move a gate by, in float64 from the inputs alone: the mean is rounded to fp32
    (|mean| EPS); each hidden value is a double sum rounded to fp32 plus a bias, two roundings of at most EPS (|sum| + |bias|) each on top
    of |w1| times the means' errors (ReLU does not stretch an error); the same for the second layer; the sigmoid has slope <= 1/4 and is
    itself expf, 1 + e and a division, taken as 4 EPS of a value <= 1."""
    t, w1, b1, w2, b2 = (v.double() for v in (t, w1, b1, w2, b2))
    m = t.mean(1)
    dm = m.abs() * EPS
    a1 = m @ w1.T
    dh = dm @ w1.abs().T + 2 * EPS * (a1.abs() + b1.abs())
    h = torch.relu(a1 + b1)
    dv = dh @ w2.abs().T + 2 * EPS * ((h @ w2.T).abs() + b2.abs())
    return 0.25 * dv + 4 * EPS


@pytest.mark.parametrize("B,HW,C,Cs", [(2, 150, 32, 4), (1, 1000, 7, 1), (1, 257, 180, 6), (3, 300, 300, 10), (1, 64, 520, 260)])
def test_channel_attention_and_combine_against_float64(B, HW, C, Cs):
    """pool -> squeeze MLP -> sigmoid -> x += (t y) conv_scale as a HAB runs them.  The updated x is held to the project's bar.  The gates
    themselves are a few fp32 roundings from exact, where a ratio of two errors is noise: they are held to _gate_bound."""
    from xmm_superres_denoise.engine import hat_ca_combine
    x, t, w1, b1, w2, b2 = _ca_inputs(B, HW, C, Cs)
    scale = 0.5
    what = f"channel attention + combine {B} x {HW} x {C}, squeezed to {Cs}"
    xs, guard = _guarded((B, HW, C))
    xs.copy_(x)
    gates, gguard = _guarded((B, C))
    hat_ca_combine(xs, t, w1, b1, w2, b2, scale, gates=gates)
    assert torch.isfinite(xs).all() and torch.isfinite(gates).all() and _untouched(guard) and _untouched(gguard), what
    x64, y64 = _ca_reference(x.double(), t.double(), w1.double(), b1.double(), w2.double(), b2.double(), scale)
    x32, y32 = _ca_reference(x, t, w1, b1, w2, b2, scale)
    _assert_within_2x_of_fp32(xs, x32, x64, what)
    gerr, bound = (gates.double() - y64).abs(), _gate_bound(t, w1, b1, w2, b2)
    print(f"{what}: gates max err {gerr.max().item():.3e} (fp32 reference {(y32.double() - y64).abs().max().item():.3e}), "
          f"largest err / bound {(gerr / bound).max().item():.3f}")
    assert torch.all(gerr <= bound), what
    again = x.clone()
    hat_ca_combine(again, t, w1, b1, w2, b2, scale)
    assert torch.equal(again, xs)                                    # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        one = x[i:i + 1].clone()
        hat_ca_combine(one, t[i:i + 1].contiguous(), w1, b1, w2, b2, scale)
        assert torch.equal(one[0], xs[i]), i


@pytest.mark.parametrize("B,HW,C", [(2, 150, 32), (1, 257, 180)])
def test_plain_combine_against_float64(B, HW, C):
    """x += t * scale, the identity branches' use of the combine: the yardstick does the same two roundings"""
    from xmm_superres_denoise.engine import hat_ca_combine
    x, t, *_ = _ca_inputs(B, HW, C, 1)
    xs, guard = _guarded((B, HW, C))
    xs.copy_(x)
    hat_ca_combine(xs, t, scale=0.75)
    assert torch.isfinite(xs).all() and _untouched(guard)
    _assert_within_2x_of_fp32(xs, x + t * 0.75, x.double() + t.double() * 0.75, f"plain combine {B} x {HW} x {C}")
    again = x.clone()
    assert torch.equal(hat_ca_combine(again, t, scale=0.75), xs)
    one = x[:1].clone()
    assert torch.equal(hat_ca_combine(one, t[:1].contiguous(), scale=0.75)[0], xs[0])


def test_channel_attention_keeps_a_nan_in_its_image():
    from xmm_superres_denoise.engine import hat_ca_combine
    x, t, w1, b1, w2, b2 = _ca_inputs(3, 300, 300, 10)
    clean = x.clone()
    hat_ca_combine(clean, t, w1, b1, w2, b2, 0.5)
    tn = t.clone()
    tn[1, 17, 5] = float("nan")
    dirty = x.clone()
    hat_ca_combine(dirty, tn, w1, b1, w2, b2, 0.5)
    assert not torch.isfinite(dirty[1]).all()
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[2], clean[2])


# ---------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched for a refused shape
# ---------------------------------------------------------------------------------------------------------------
def _attn_args(B=1, H=8, W=8, C=8, heads=2, ws=4, shift=0):
    return (torch.zeros(B, H * W, 3 * C, device="cuda"), torch.zeros((2 * ws - 1) ** 2, heads, device="cuda"), H, W, heads, ws, shift, 1.0)


@pytest.mark.parametrize("kw,msg", [
    (dict(ws=17, H=17, W=17), r"window size 17 is outside \[1, 16\]"),
    (dict(H=10), "H and W must be multiples of the window size 4; got 10 x 8"),
    (dict(W=6), "H and W must be multiples of the window size 4; got 8 x 6"),
    (dict(shift=4), r"shift 4 is outside \[0, window size 4\)"),
    (dict(shift=-1), r"shift -1 is outside \[0, window size 4\)"),
    (dict(C=66, heads=2), "head dim 33; the kernel takes at most 32"),
    (dict(C=9, heads=2), "2 heads do not divide 9 channels"),
])
def test_window_attention_refusals(kw, msg):
    from xmm_superres_denoise.engine import XsdError, sw_window_attention
    with pytest.raises(XsdError, match=msg):
        sw_window_attention(*_attn_args(**kw))


def test_window_attention_refusals_of_the_library_itself():
    """what the wrapper cannot express goes through the C entry point; the pointers are valid and nothing is launched"""
    from xmm_superres_denoise.engine import _lib
    L, t = _lib.load(), torch.zeros(64, device="cuda")
    p = t.data_ptr()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert L.xsd_sw_test_attention(p, p, p, B, H, W, 8, 2, 4, 0, 1.0, None) != 0
        assert f"window attention test: bad shape {B}x{H}x{W}".encode() in L.xsd_last_error()
    assert L.xsd_sw_test_attention(p, p, p, 1, 16400, 16400, 8, 2, 16, 0, 1.0, None) != 0         # 16400^2 > 2^28 tokens
    assert b"1 images of 16400 x 16400 tokens are too many" in L.xsd_last_error()
    assert L.xsd_sw_test_attention(p, p, p, 65, 2048, 2048, 8, 2, 1, 0, 1.0, None) != 0           # 65 * 2^22 > 2^28 tokens
    assert b"65 images of 2048 x 2048 tokens are too many" in L.xsd_last_error()
    assert L.xsd_sw_test_attention(p, p, p, 1, 8, 8, 8, 0, 4, 0, 1.0, None) != 0
    assert b"0 heads do not divide 8 channels" in L.xsd_last_error()
    for q, tb, o in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.xsd_sw_test_attention(q, tb, o, 1, 8, 8, 8, 2, 4, 0, 1.0, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert torch.all(t == 0)


def test_layernorm_and_combine_refusals_of_the_library_itself():
    from xmm_superres_denoise.engine import _lib
    L, t = _lib.load(), torch.zeros(64, device="cuda")
    p = t.data_ptr()
    for M in (0, -3, (1 << 31) + 1):
        assert L.xsd_sw_test_layernorm(p, p, p, p, M, 8, None) != 0
        assert f"LayerNorm test: {M} rows are outside [1, 2^31]".encode() in L.xsd_last_error()
    assert L.xsd_sw_test_layernorm(p, p, p, p, 4, 0, None) != 0
    assert b"LayerNorm test: 0 channels are outside [1, 4096]" in L.xsd_last_error()
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.xsd_sw_test_layernorm(*a, 4, 8, None) != 0
        assert b"null argument" in L.xsd_last_error()
    # HAT combine: (x, t, w1, b1, w2, b2, scale, B, HW, C, Cs, gates, stream)
    for HW in (0, (1 << 28) + 1):
        assert L.xsd_hat_test_ca_combine(p, p, None, None, None, None, 1.0, 1, HW, 8, 0, None, None) != 0
        assert f"HAT combine test: {HW} pixels are outside [1, 2^28]".encode() in L.xsd_last_error()
    assert L.xsd_hat_test_ca_combine(p, p, None, None, None, None, 1.0, 0, 4, 8, 0, None, None) != 0
    assert b"HAT combine test: 0 images are outside [1, 65535]" in L.xsd_last_error()
    assert L.xsd_hat_test_ca_combine(p, p, None, None, None, None, 1.0, 1, 4, 0, 0, None, None) != 0
    assert b"HAT combine test: 0 channels are outside [1, 4096]" in L.xsd_last_error()
    assert L.xsd_hat_test_ca_combine(p, p, None, None, None, None, 1.0, 1025, 1 << 28, 1, 0, None, None) != 0      # 1025 * 2^28 > 2^38
    assert b"HAT combine test: 1025 x 268435456 x 1 elements are too many" in L.xsd_last_error()
    for w1, b1, w2, b2 in ((p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.xsd_hat_test_ca_combine(p, p, w1, b1, w2, b2, 1.0, 1, 4, 8, 2, None, None) != 0
        assert b"the squeeze MLP needs both weights and both biases" in L.xsd_last_error()
    assert L.xsd_hat_test_ca_combine(p, p, p, p, p, p, 1.0, 1, 4, 8, 0, None, None) != 0
    assert b"a squeezed width of 0 is outside [1, 4096]" in L.xsd_last_error()
    for x, tt in ((None, p), (p, None)):
        assert L.xsd_hat_test_ca_combine(x, tt, None, None, None, None, 1.0, 1, 4, 8, 0, None, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert torch.all(t == 0)


def test_layernorm_and_combine_refusals():
    from xmm_superres_denoise.engine import XsdError, hat_ca_combine, sw_layernorm
    z = torch.zeros
    with pytest.raises(XsdError, match=r"4097 channels are outside \[1, 4096\]"):
        sw_layernorm(z(2, 4097, device="cuda"), z(4097, device="cuda"), z(4097, device="cuda"))
    x = z(1, 4, 4097, device="cuda")
    with pytest.raises(XsdError, match=r"HAT combine test: 4097 channels are outside \[1, 4096\]"):
        hat_ca_combine(x, x.clone())
    x = z(1, 4, 8, device="cuda")
    with pytest.raises(XsdError, match=r"a squeezed width of 4097 is outside \[1, 4096\]"):
        hat_ca_combine(x, x.clone(), z(4097, 8, device="cuda"), z(4097, device="cuda"), z(8, 4097, device="cuda"), z(8, device="cuda"))
    with pytest.raises(XsdError, match="no gates to return without the squeeze weights"):
        hat_ca_combine(x, x.clone(), gates=z(1, 8, device="cuda"))
    many = z(65536, 1, 1, device="cuda")
    with pytest.raises(XsdError, match=r"65536 images are outside \[1, 65535\]"):
        hat_ca_combine(many, many.clone())
    assert torch.all(x == 0)


# ---------------------------------------------------------------------------------------------------------------
# whole networks at SwinFIR's published window of 12 (5 tiles per window)
# ---------------------------------------------------------------------------------------------------------------
W12 = dict(img_size=24, patch_size=1, in_chans=1, embed_dim=60, depths=[2], num_heads=[2], window_size=12, upsampler="pixelshuffle")


def _sd(state, dtype):
    return {k: torch.from_numpy(v).cuda().to(dtype) if v.dtype == np.float32 else torch.from_numpy(v).cuda() for k, v in state.items()}


def test_swinfir_with_window_12_in_both_math_modes():
    from xmm_superres_denoise.models import SwinFIR
    state = gs.make_state(W12, 51)
    m = SwinFIR(**gs.full_cfg(**W12))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    m = m.cuda()
    x = torch.from_numpy(gs.make_input((1, 1, 24, 36), 52)).cuda()
    with torch.no_grad():
        y = m(x)
        y6 = m.set_math("bf16x6")(x)
        y64 = st.swinfir_forward(_sd(state, torch.float64), x.double(), **W12)
        y32 = st.swinfir_forward(_sd(state, torch.float32), x, **W12)
    assert y.shape == y64.shape == (1, 1, 48, 72) and not torch.equal(y, y6)
    _assert_within_2x_of_fp32(y, y32, y64, "SwinFIR window 12, 24 x 36, fp32")
    _assert_within_2x_of_fp32(y6, y32, y64, "SwinFIR window 12, 24 x 36, bf16x6")


def test_hat_with_window_12_and_overlap_18():
    from xmm_superres_denoise.models import HAT
    cfg = dict(W12, overlap_ratio=0.5)
    state = gh.make_state(cfg, 53)
    m = HAT(**gh.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    m = m.cuda()
    x = torch.from_numpy(gh.make_input((1, 1, 24, 24), 54)).cuda()
    with torch.no_grad():
        y = m(x)
        y64 = ht.hat_forward(_sd(state, torch.float64), x.double(), **cfg)
        y32 = ht.hat_forward(_sd(state, torch.float32), x, **cfg)
    assert y.shape == y64.shape == (1, 1, 48, 48)
    _assert_within_2x_of_fp32(y, y32, y64, "HAT window 12 / 18, 24 x 24")
