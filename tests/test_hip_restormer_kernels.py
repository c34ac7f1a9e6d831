"""The Restormer engine's kernels (csrc/restormer.hip), each on its own through its test hook (include/xsd.h) against a plain float64
reference of the same operation: the 1x1 conv with its fused LayerNorm, per-image weights, residual and slab strides; the depthwise 3x3
with its GELU gate; the channel attention (Gram, softmax, folded project_out) up to 64 channels per head, at one channel per head, over
a ragged second pixel range and over a single pixel; the dense 3x3 with its two pixel-shuffle stores; then two whole networks that
reach those corners.  The yardstick is the same reference in fp32 on the same device, the bar the project's 2x.  Every output buffer is
pre-filled (NaN where the kernel must write, a finite sentinel in guard elements behind it or in the channels it must leave alone)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_restormer as gr
import restormer_torch as rt

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    y, y32, y64 = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (y, y32, y64))
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


def _guarded(shape, guard=300):
    """a NaN-filled contiguous tensor of `shape` with `guard` sentinel elements behind it in the same allocation"""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), SENTINEL, device="cuda")
    buf[:n] = float("nan")
    return buf[:n].view(shape), buf[n:]


def _untouched(guard):
    return bool(torch.all(guard == SENTINEL))


def _u(g, *shape, fan):
    return ((torch.rand(*shape, generator=g) * 2 - 1) / fan ** 0.5).cuda()


# ---------------------------------------------------------------------------------------------------------------
# 1x1 conv
# ---------------------------------------------------------------------------------------------------------------
def _pw_reference(x, w, bias, ln, lnw, lnb, res):
    if ln:
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        x = (x - mu) / torch.sqrt(var + 1e-5) * lnw[:, None] + lnb[:, None] if ln == "WithBias" else x / torch.sqrt(var + 1e-5) * lnw[:, None]
    y = torch.matmul(w, x)                                           # [(B,) cout, cin] @ [B, cin, HW]
    if bias is not None:
        y = y + bias[:, None]
    return y if res is None else res + y


def _pw_inputs(B, cin, cout, HW, ln, per_image, bias, residual):
    g = torch.Generator().manual_seed(10000 * cin + 100 * cout + HW)
    x = (torch.randn(B, cin, HW, generator=g) * 2 + 0.3).cuda()
    w = _u(g, *((B, cout, cin) if per_image else (cout, cin)), fan=cin) * 1.7
    b = _u(g, cout, fan=1) if bias else None
    lnw = (1 + 0.4 * (torch.rand(cin, generator=g) - 0.5)).cuda() if ln else None
    lnb = (0.4 * (torch.rand(cin, generator=g) - 0.5)).cuda() if ln == "WithBias" else None
    res = torch.randn(B, cout, HW, generator=g).cuda() if residual else None
    return x, w, b, lnw, lnb, res


def _d(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("B,cin,cout,HW,ln,per_image,bias,residual", [
    (2, 24, 72, 100, "WithBias", False, False, False),
    (1, 33, 65, 63, "BiasFree", False, True, False),                 # every tile edge off
    (2, 48, 48, 130, None, True, True, True),                        # the attention's folded per-image matrix, added in place
    (1, 2, 5, 7, "WithBias", False, False, False),
    (1, 192, 384, 20, "WithBias", False, True, False),
    (1, 21, 8, 70, None, False, True, True),
])
def test_pointwise_conv_against_float64(B, cin, cout, HW, ln, per_image, bias, residual):
    from xmm_superres_denoise.engine import restormer_pw
    x, w, b, lnw, lnb, res = _pw_inputs(B, cin, cout, HW, ln, per_image, bias, residual)
    what = f"1x1 {B} x {cin} -> {cout} x {HW}, ln {ln}, per-image {per_image}, bias {bias}, residual {residual}"

    def run(x, w, res):
        out, guard = _guarded((x.shape[0], cout, HW))
        if res is not None:
            out.copy_(res)
        y = restormer_pw(x, w, b, ln, lnw, lnb, residual, out=out)
        assert torch.isfinite(y).all() and _untouched(guard), what
        return y

    y = run(x, w, res)
    y64 = _pw_reference(x.double(), w.double(), _d(b), ln, _d(lnw), _d(lnb), _d(res))
    y32 = _pw_reference(x, w, b, ln, lnw, lnb, res)
    _assert_within_2x_of_fp32(y, y32, y64, what)
    assert torch.equal(run(x, w, res), y)                            # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        one = run(x[i:i + 1].contiguous(), w[i:i + 1].contiguous() if per_image else w, None if res is None else res[i:i + 1])
        assert torch.equal(one[0], y[i]), i


def test_pointwise_conv_on_a_channel_prefix_of_a_wider_slab():
    """what the decoder does: the first 24 of a slab's 40 channels in, the first 36 of another slab's 50 channels out, through the batch
    strides; the other output channels keep their sentinel"""
    from xmm_superres_denoise.engine import restormer_pw
    B, cin, cout, HW, Cx, Cy = 2, 24, 36, 70, 40, 50
    x, w, b, lnw, lnb, _ = _pw_inputs(B, Cx, cout, HW, "WithBias", False, True, False)
    w, lnw, lnb = w[:, :cin].contiguous(), lnw[:cin].contiguous(), lnb[:cin].contiguous()
    slab, guard = _guarded((B, Cy, HW))
    slab[:, cout:] = SENTINEL
    restormer_pw(x, w, b, "WithBias", lnw, lnb, out=slab)
    assert torch.isfinite(slab).all() and torch.all(slab[:, cout:] == SENTINEL) and _untouched(guard)
    xp = x[:, :cin].contiguous()
    y64 = _pw_reference(xp.double(), w.double(), b.double(), "WithBias", lnw.double(), lnb.double(), None)
    y32 = _pw_reference(xp, w, b, "WithBias", lnw, lnb, None)
    _assert_within_2x_of_fp32(slab[:, :cout], y32, y64, "1x1 on a 24-channel prefix of 40 into a 36-channel prefix of 50")
    assert torch.equal(restormer_pw(xp, w, b, "WithBias", lnw, lnb), slab[:, :cout])      # = the same conv on packed tensors


# ---------------------------------------------------------------------------------------------------------------
# depthwise 3x3
# ---------------------------------------------------------------------------------------------------------------
def _dw_reference(x, w, b, gate):
    y = F.conv2d(x, w, b, padding=1, groups=x.shape[1])
    if gate:
        x1, x2 = y.chunk(2, dim=1)
        y = F.gelu(x1) * x2
    return y


def _dw_bound(x, w, b, gate):
    """what fp32 rounding can move an output of rst_dw_kernel by, in float64 from the inputs alone, u = 2^-24.  The conv is a chain of 9
    fmaf and a bias add: 10 roundings, each at most u times a partial sum that the sum S of the |w x| and |bias| bounds, so 10 u S.  The
    gate computes g = (0.5 v) (1 + erff(v * 0.70710678f)) v2: the argument carries 2 u |t| (the constant and the product), which erf's
    slope 1.13 exp(-t^2) turns into at most u; erff itself is taken as 2 ulp = 4 u of a value <= 1; 1 + erf <= 2 rounds by 2 u: 7 u on
    the bracket.  So dgelu <= 0.5 |v| 7 u + u |gelu| + 1.13 dv (|gelu'| <= 1.13), and the product with v2 adds |gelu| dv2 + u |gelu v2|."""
    u = 2.0 ** -24
    x, w, b = x.double(), w.double(), _d(b)
    C = x.shape[1]
    v = F.conv2d(x, w, b, padding=1, groups=C)
    dv = 10 * u * F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), padding=1, groups=C)
    if not gate:
        return dv
    (v1, v2), (d1, d2) = v.chunk(2, dim=1), dv.chunk(2, dim=1)
    gl = F.gelu(v1)
    dg = 0.5 * v1.abs() * 7 * u + u * gl.abs() + 1.13 * d1
    return v2.abs() * dg + gl.abs() * d2 + u * (gl * v2).abs()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,cout,gate,H,W", [(2, 6, False, 5, 7), (1, 21, True, 9, 33), (1, 4, True, 1, 300), (1, 3, False, 17, 1)])
def test_depthwise_conv_against_float64(B, cout, gate, H, W, bias):
    """the gate's inputs are scaled so that |x1| reaches 10, where erf has long saturated.  Nine products and a bias: the engine's
    error and the yardstick's are both a few units of 2^-24 and their ratio is noise (on the MI355X the yardstick's depthwise conv is
    correctly rounded at these sizes, 1.6e-7 rms against the engine's 3.8e-7 at 2 x 6 x 5 x 7: a ratio of 2.4 from a healthy fmaf chain),
    so both pairs are printed and the assertion is the rounding bound of _dw_bound, element by element, for every case: which cases
    would meet the 2x bar is known only from measuring them, and a bound is not chosen by what the kernel gives.  The printed ratio to
    the bound (0.09 - 0.30 on the MI355X, docs/LAB_NOTEBOOK.md 2026-10-18) is what shows a later loss of precision."""
    from xmm_superres_denoise.engine import restormer_dw
    g = torch.Generator().manual_seed(1000 * H + W)
    cin = 2 * cout if gate else cout
    x = (torch.randn(B, cin, H, W, generator=g) * 4).cuda()
    w = (torch.rand(cin, 1, 3, 3, generator=g) * 2 - 1).cuda()
    b = (torch.rand(cin, generator=g) - 0.5).cuda() if bias else None
    what = f"depthwise {B} x {cout} x {H} x {W}, gate {gate}, bias {bias}"
    out, guard = _guarded((B, cout, H, W))
    y = restormer_dw(x, w, b, gate, out=out)
    assert torch.isfinite(y).all() and _untouched(guard), what
    y64 = _dw_reference(x.double(), w.double(), _d(b), gate)
    y32 = _dw_reference(x, w, b, gate)
    if gate:
        assert F.conv2d(x.double(), w.double(), _d(b), padding=1, groups=cin)[:, :cout].abs().max() >= 10
    (rms, mx), (rms32, mx32) = _errs(y.cpu().numpy(), y64.cpu().numpy()), _errs(y32.cpu().numpy(), y64.cpu().numpy())
    ratio = float(((y.double() - y64).abs() / _dw_bound(x, w, b, gate)).max())
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e} | largest err / rounding bound "
          f"{ratio:.3f}")
    assert ratio <= 1, (what, ratio)
    assert torch.equal(restormer_dw(x, w, b, gate), y)               # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        assert torch.equal(restormer_dw(x[i:i + 1].contiguous(), w, b, gate)[0], y[i]), i


# ---------------------------------------------------------------------------------------------------------------
# channel attention
# ---------------------------------------------------------------------------------------------------------------
def _attn_inputs(B, C, heads, HW):
    g = torch.Generator().manual_seed(10000 * C + 100 * heads + HW)
    qkv = torch.randn(B, 3 * C, HW, generator=g).cuda()
    temp = torch.rand(heads, generator=g) * 1.5 + 0.5
    if heads > 1:
        temp[-1] = -temp[-1]
    wpo = _u(g, C, C, fan=C)
    bpo = _u(g, C, fan=1) if heads > 1 else None
    x = torch.randn(B, C, HW, generator=g).cuda()
    return qkv, temp.cuda(), wpo, bpo, x


def _attn_reference(qkv, temp, wpo, bpo, x, heads):
    B, C, HW = x.shape
    o = rt.channel_attention(qkv.view(B, 3 * C, HW, 1), temp.view(heads, 1, 1), heads).view(B, C, HW)
    y = torch.matmul(wpo, o)
    return x + (y if bpo is None else y + bpo[:, None])


ATTN_CASES = [
    (2, 64, 1, 1500),        # 64 channels per head, a second range of 476 pixels
    (1, 6, 6, 70),           # one channel per head: every softmax is over one logit
    (2, 15, 3, 1),           # a single pixel: F.normalize divides a one-element row
    (1, 48, 1, 1024),        # exactly one range
    (1, 48, 2, 1025),        # a second range of one pixel
    (1, 40, 8, 3000),
]


@pytest.mark.parametrize("B,C,heads,HW", ATTN_CASES)
def test_channel_attention_against_float64(B, C, heads, HW):
    from xmm_superres_denoise.engine import restormer_channel_attention
    qkv, temp, wpo, bpo, x = _attn_inputs(B, C, heads, HW)
    if HW == 1025:
        qkv[0, 3] = 0            # a q channel that is zero over the whole image: its norm is clamped at 1e-12
    what = f"channel attention {B} x {C} ({heads} heads) x {HW}"

    def run(qkv, x):
        xs, guard = _guarded(tuple(x.shape))
        xs.copy_(x)
        restormer_channel_attention(qkv, temp, wpo, bpo, xs, heads)
        assert torch.isfinite(xs).all() and _untouched(guard), what
        return xs

    y = run(qkv, x)
    y64 = _attn_reference(qkv.double(), temp.double(), wpo.double(), _d(bpo), x.double(), heads)
    y32 = _attn_reference(qkv, temp, wpo, bpo, x, heads)
    _assert_within_2x_of_fp32(y, y32, y64, what)
    assert torch.equal(run(qkv, x), y)                               # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        assert torch.equal(run(qkv[i:i + 1].contiguous(), x[i:i + 1].contiguous())[0], y[i]), i


def test_channel_attention_keeps_a_nan_in_its_image():
    from xmm_superres_denoise.engine import restormer_channel_attention
    B, C, heads, HW = ATTN_CASES[0]
    qkv, temp, wpo, bpo, x = _attn_inputs(B, C, heads, HW)
    clean = restormer_channel_attention(qkv, temp, wpo, bpo, x.clone(), heads)
    qn = qkv.clone()
    qn[1, 70, 1234] = float("nan")           # a k channel of image 1
    dirty = restormer_channel_attention(qn, temp, wpo, bpo, x.clone(), heads)
    assert not torch.isfinite(dirty[1]).all()
    assert torch.equal(dirty[0], clean[0])


# ---------------------------------------------------------------------------------------------------------------
# dense 3x3 conv
# ---------------------------------------------------------------------------------------------------------------
def _c3_reference(x, w, b, skip, mode):
    y = F.conv2d(x, w, b, padding=1)
    if mode == "unshuffle":
        return F.pixel_unshuffle(y, 2)
    if mode == "shuffle":
        return F.pixel_shuffle(y, 2)
    return y if skip is None else y + skip


@pytest.mark.parametrize("B,cin,cout,H,W,mode,extras", [
    (1, 1, 24, 17, 33, None, False),
    (2, 16, 3, 16, 16, None, True),          # bias and skip: the output conv
    (1, 9, 10, 1, 40, None, False),
    (2, 24, 12, 10, 22, "unshuffle", False),
    (1, 20, 40, 5, 7, "shuffle", False),
])
def test_conv3x3_against_float64(B, cin, cout, H, W, mode, extras):
    from xmm_superres_denoise.engine import restormer_conv3x3
    g = torch.Generator().manual_seed(10000 * cin + 100 * H + W)
    x = torch.randn(B, cin, H, W, generator=g).cuda()
    w = _u(g, cout, cin, 3, 3, fan=9 * cin) * 1.7
    b = _u(g, cout, fan=1) if extras else None
    skip = torch.randn(B, cout, H, W, generator=g).cuda() if extras else None
    what = f"3x3 {B} x {cin} -> {cout} x {H} x {W}, mode {mode}, bias and skip {extras}"
    y64 = _c3_reference(x.double(), w.double(), _d(b), _d(skip), mode)
    y32 = _c3_reference(x, w, b, skip, mode)
    out, guard = _guarded(tuple(y64.shape))
    y = restormer_conv3x3(x, w, b, skip, mode, out=out)
    assert torch.isfinite(y).all() and _untouched(guard), what
    _assert_within_2x_of_fp32(y, y32, y64, what)
    assert torch.equal(restormer_conv3x3(x, w, b, skip, mode), y)    # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        one = restormer_conv3x3(x[i:i + 1].contiguous(), w, b, None if skip is None else skip[i:i + 1].contiguous(), mode)
        assert torch.equal(one[0], y[i]), i


# ---------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched for a refused shape
# ---------------------------------------------------------------------------------------------------------------
def _z(*shape):
    return torch.zeros(*shape, device="cuda")


def test_pointwise_conv_refusals():
    from xmm_superres_denoise.engine import XsdError, _lib, restormer_pw
    with pytest.raises(XsdError, match=r"Restormer 1x1 test: 65536 images are outside \[1, 65535\]"):
        restormer_pw(_z(65536, 1, 1), _z(1, 1))
    with pytest.raises(XsdError, match=r"131073 -> 1 channels are outside \[1, 131072\]"):
        restormer_pw(_z(1, 131073, 1), _z(1, 131073))
    with pytest.raises(XsdError, match=r"1 -> 131073 channels are outside \[1, 131072\]"):
        restormer_pw(_z(1, 1, 1), _z(131073, 1))
    with pytest.raises(XsdError, match="LayerNorm mode 1 needs its weight and bias"):
        restormer_pw(_z(1, 4, 8), _z(4, 4), ln="WithBias", ln_weight=_z(4))
    with pytest.raises(XsdError, match="LayerNorm mode 2 needs its weight"):
        restormer_pw(_z(1, 4, 8), _z(4, 4), ln="BiasFree")
    # what the wrapper cannot express goes through the C entry point itself; the pointers are valid and nothing is launched
    L, t = _lib.load(), _z(64)
    p = t.data_ptr()
    assert L.xsd_restormer_test_pw(p, 32, p, 0, None, 3, p, p, 0, p, 32, 1, 4, 4, 8, None) != 0
    assert b"LayerNorm mode 3 is not 0 (none), 1 (WithBias) or 2 (BiasFree)" in L.xsd_last_error()
    assert L.xsd_restormer_test_pw(p, 31, p, 0, None, 0, None, None, 0, p, 32, 1, 4, 4, 8, None) != 0
    assert b"batch strides 31 / 32 are smaller than the 4 / 4 channels of 8 pixels" in L.xsd_last_error()
    assert L.xsd_restormer_test_pw(p, 32, p, 0, None, 0, None, None, 0, p, 32, 1, 4, 4, (1 << 28) + 1, None) != 0
    assert b"268435457 pixels are outside [1, 2^28]" in L.xsd_last_error()
    for x, w, y in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.xsd_restormer_test_pw(x, 32, w, 0, None, 0, None, None, 0, y, 32, 1, 4, 4, 8, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert torch.all(t == 0)


def test_depthwise_conv_refusals():
    from xmm_superres_denoise.engine import XsdError, _lib, restormer_dw
    with pytest.raises(XsdError, match=r"65536 output channels are outside \[1, 65535\]"):
        restormer_dw(_z(1, 65536, 1, 1), _z(65536, 1, 3, 3))
    with pytest.raises(XsdError, match=r"Restormer depthwise test: 65536 images are outside \[1, 65535\]"):
        restormer_dw(_z(65536, 1, 1, 1), _z(1, 1, 3, 3))
    L, t = _lib.load(), _z(64)
    p = t.data_ptr()
    assert L.xsd_restormer_test_dw(p, p, None, p, 1, 2, 2, 2, 2, None) != 0
    assert b"mode 2 is not 0 (plain) or 1 (gate)" in L.xsd_last_error()
    assert L.xsd_restormer_test_dw(p, p, None, p, 1, 2, 0, 0, 2, None) != 0
    assert b"bad image size 0 x 2" in L.xsd_last_error()
    assert L.xsd_restormer_test_dw(p, p, None, p, 1, 1, 0, 1 << 15, 1 << 14, None) != 0
    assert b"536870912 pixels are outside [1, 2^28]" in L.xsd_last_error()
    for x, w, y in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.xsd_restormer_test_dw(x, w, None, y, 1, 2, 0, 2, 2, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert torch.all(t == 0)


def test_channel_attention_refusals():
    from xmm_superres_denoise.engine import XsdError, _lib, restormer_channel_attention
    with pytest.raises(XsdError, match="65 channels per head; the kernels take at most 64"):
        restormer_channel_attention(_z(1, 195, 4), _z(1), _z(65, 65), None, _z(1, 65, 4), 1)
    with pytest.raises(XsdError, match="3 heads do not divide 10 channels"):
        restormer_channel_attention(_z(1, 30, 4), _z(3), _z(10, 10), None, _z(1, 10, 4), 3)
    with pytest.raises(XsdError, match=r"Restormer attention test: 65536 images are outside \[1, 65535\]"):
        restormer_channel_attention(_z(65536, 3, 1), _z(1), _z(1, 1), None, _z(65536, 1, 1), 1)
    L, t = _lib.load(), _z(64)
    p = t.data_ptr()
    assert L.xsd_restormer_test_attention(p, p, p, None, p, 1, 8256, 129, 4, None) != 0
    assert b"8256 channels are outside [1, 8192]" in L.xsd_last_error()
    assert L.xsd_restormer_test_attention(p, p, p, None, p, 1, 4, 1, 0, None) != 0
    assert b"0 pixels are outside [1, 2^28]" in L.xsd_last_error()
    assert L.xsd_restormer_test_attention(p, p, p, None, p, 1, 4, 0, 4, None) != 0
    assert b"0 heads do not divide 4 channels" in L.xsd_last_error()
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.xsd_restormer_test_attention(a[0], a[1], a[2], None, a[3], 1, 4, 2, 4, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert torch.all(t == 0)


def test_conv3x3_refusals():
    from xmm_superres_denoise.engine import XsdError, _lib, restormer_conv3x3
    # a shape without an output shape never leaves the wrapper ...
    with pytest.raises(XsdError, match="PixelUnshuffle.* of 5 x 4 has no output shape"):
        restormer_conv3x3(_z(1, 2, 5, 4), _z(2, 2, 3, 3), mode="unshuffle")
    with pytest.raises(XsdError, match="PixelShuffle.* of 6 channels has no output shape"):
        restormer_conv3x3(_z(1, 2, 4, 4), _z(6, 2, 3, 3), mode="shuffle")
    with pytest.raises(XsdError, match="the skip is added in the plain mode only"):
        restormer_conv3x3(_z(1, 2, 4, 4), _z(4, 2, 3, 3), skip=_z(1, 4, 4, 4), mode="shuffle")
    with pytest.raises(XsdError, match=r"Restormer 3x3 test: 65536 images are outside \[1, 65535\]"):
        restormer_conv3x3(_z(65536, 1, 1, 1), _z(1, 1, 3, 3))
    # ... and the library refuses it by itself
    L, t = _lib.load(), _z(64)
    p = t.data_ptr()
    for H, W in ((5, 4), (4, 5)):
        assert L.xsd_restormer_test_conv3(p, p, None, None, p, 1, 1, 1, H, W, 1, None) != 0
        assert f"PixelUnshuffle(2) needs even H and W; got {H} x {W}".encode() in L.xsd_last_error()
    assert L.xsd_restormer_test_conv3(p, p, None, None, p, 1, 1, 6, 2, 2, 2, None) != 0
    assert b"PixelShuffle(2) needs a multiple of 4 output channels; got 6" in L.xsd_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.xsd_restormer_test_conv3(args[0], args[1], None, None, args[2], 1, 1, 1, 2, 2, 0, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert L.xsd_restormer_test_conv3(p, p, None, None, p, 1, 131073, 1, 1, 1, 0, None) != 0
    assert b"131073 -> 1 channels are outside [1, 131072]" in L.xsd_last_error()
    assert L.xsd_restormer_test_conv3(p, p, None, None, p, 1, 1, 1, 2, 2, 3, None) != 0
    assert b"mode 3 is not 0 (plain), 1 (PixelUnshuffle) or 2 (PixelShuffle)" in L.xsd_last_error()
    assert L.xsd_restormer_test_conv3(p, p, None, None, p, 1, 1, 1, 2, 0, 0, None) != 0
    assert b"bad image size 2 x 0" in L.xsd_last_error()
    assert torch.all(t == 0)


# ---------------------------------------------------------------------------------------------------------------
# whole networks that reach the corners above
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg,shape", [
    # the latent level is one pixel: its attention normalizes one-element rows, its depthwise convs see only padding around it
    ("8 x 8", dict(inp_channels=1, out_channels=1, dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 2, 4, 8]), (2, 1, 8, 8)),
    # decoder_level1 and the refinement run 2 dim = 64 channels on heads[0] = 1 head
    ("64 channels per head", dict(inp_channels=1, out_channels=1, dim=32, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 2, 4, 8]),
     (1, 1, 16, 16)),
])
def test_whole_network_against_float64_restatement(name, cfg, shape):
    from xmm_superres_denoise.models import Restormer
    state = gr.make_state(cfg, 61)
    m = Restormer(**gr.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    m = m.cuda()
    x = torch.from_numpy(gr.make_input(shape, 62)).cuda()
    full = gr.full_cfg(**cfg)
    with torch.no_grad():
        y = m(x)
        y64 = rt.restormer_forward({k: torch.from_numpy(v).cuda().double() for k, v in state.items()}, x.double(), **full)
        y32 = rt.restormer_forward({k: torch.from_numpy(v).cuda() for k, v in state.items()}, x, **full)
    assert y.shape == y64.shape == shape
    _assert_within_2x_of_fp32(y, y32, y64, f"Restormer {name}")
