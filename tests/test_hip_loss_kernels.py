"""The 14 kernels of csrc/loss_kernels.hip below the whole terms: one SSIM scale alone (xsd_loss_test_scale: the two host functions the
SSIM / MS-SSIM chain runs per scale), the pooling alone (xsd_loss_test_pool2), and xsd_loss_eval at the shapes and inputs where its
reductions, selects and size checks take their other branches.

Reference: oracle/loss.py in float64.  Bars, those of tests/test_hip_loss.py: values 2e-6 max(1, |v|), gradients 2e-5 max|g|, per tensor
and, for the one-scale entry, per image.  Whatever is called exact compares bits.
Every tensor of a launch lies between NaN guard bands in one allocation (util_hip.Guarded), outputs start as NaN unless accumulating,
read-only tensors must come back bit for bit.  Inputs come from make_golden_loss.loss_inputs unless stated."""
import ctypes

import numpy as np
import pytest
import torch

import make_golden_loss as mg
from oracle import loss as ol
from util_hip import Guarded

pytestmark = pytest.mark.gpu

VAL_RTOL, GRAD_TOL = 2e-6, 2e-5
SCAL = ("pmin", "pmax", "tmin", "tmax", "dr", "c1", "c2", "from_p", "nmax", "nmin", "ddr")
WORST = {}


@pytest.fixture(scope="module")
def L():
    from xmm_superres_denoise.engine import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def note(family, what, err, bar):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"{family} {what}: error {err:.3e}, bar {bar:.3e}: {ratio:.3f} of the bar (worst {family} so far {WORST[family]:.3f})")
    return ratio


def hold_value(family, what, got, ref):
    err, bar = abs(float(got) - float(ref)), VAL_RTOL * max(1.0, abs(float(ref)))
    note(family, what, err, bar)
    assert err <= bar, f"{family} {what}: {got!r} against {ref!r}: {err:.3e} > {bar:.3e}"


def hold_grad(family, what, got, ref, zero_where_ref_is=False, ref32=None):
    """ref32 (the ill-conditioned cases only, see scale_f32): the bar becomes max(project bar, 2 max|f32 - f64|)"""
    ref = np.asarray(ref, np.float64)
    err, bar = float(np.abs(got - ref).max()), GRAD_TOL * float(np.abs(ref).max())
    if ref32 is not None:
        own = float(np.abs(np.asarray(ref32, np.float64) - ref).max())
        print(f"{family} {what}: numpy float32 against float64 {own:.3e}, project bar {bar:.3e}")
        bar = max(bar, 2 * own)
    note(family, what, err, bar)
    assert err <= bar, f"{family} {what}: {err:.3e} > {bar:.3e}"
    if zero_where_ref_is:
        assert not got[ref == 0].any(), f"{family} {what}: a gradient where the float64 reference has exactly none"


def loss_cfg(sigma=2.5, k1=0.01, k2=0.05, **w):
    from xmm_superres_denoise.utils.loss_functions import _LossConfigC
    return _LossConfigC(w.get("l1", 0.0), w.get("poisson", 0.0), w.get("psnr", 0.0), w.get("ssim", 0.0), w.get("ms_ssim", 0.0), 0.0, sigma, k1, k2, 13)


def scale_f32(p, t, gup, sigma, k1=0.01, k2=0.05):
    """oracle.ssim_scale's own formulas in numpy float32 (images, taps, constants): d/dp for the upstream pair gup [B][2].  The measure of
    a case's conditioning: sigma = 0.3 is a 3-tap window with 0.4 % of its weight off the centre, so a window's variance is ~1e-4, far
    below c2 = 2.5e-3, and the gradient maps divide fp32 roundings of the moments by it."""
    from unittest import mock
    taps = ol.gaussian_taps(sigma).astype(np.float32)
    with mock.patch.object(ol, "gaussian_taps", lambda _sigma: taps):
        _, _, back = ol.ssim_scale(p.astype(np.float32), t.astype(np.float32), sigma, np.float32(k1), np.float32(k2))
    gup = np.asarray(gup, np.float32).reshape(len(p), 2)
    return back(gup[:, 0], gup[:, 1])


def span01(B, H, W, seed):
    """loss_inputs with 0 and 1 planted in both images (small images need not reach the clip bounds): both ranges are exactly 1"""
    p, t = mg.loss_inputs(B, H, W, seed)
    if H * W >= 4:
        p[0, 0, 0], p[B - 1, H - 1, W - 1], t[0, 0, W - 1], t[B - 1, H - 1, 0] = 0.0, 1.0, 1.0, 0.0
    return p, t


# =====================================================================================================================================
# one SSIM scale
# =====================================================================================================================================

def run_scale(L, p, t, gup=None, coarse=None, dy0=None, sigma=2.5, k1=0.01, k2=0.05, expect_rc=0):
    """xsd_loss_test_scale between guard bands -> (stat [B][2] float64, {scalar: value}, dy or None)"""
    B, H, W = p.shape
    items = dict(y=p, t=t, stat=(4 * B,))
    ro = ["y", "t"]
    if gup is not None:
        items["gup"] = np.asarray(gup, np.float32)
        items["dy"] = dy0 if dy0 is not None else (B, H, W)
        ro.append("gup")
    if coarse is not None:
        items["coarse"] = coarse
        ro.append("coarse")
    g = Guarded(ro=ro, **items)
    scal = (ctypes.c_float * 11)(*([float("nan")] * 11))
    cfg = loss_cfg(sigma, k1, k2, ssim=1.0)
    rc = L.xsd_loss_test_scale(ctypes.byref(cfg), g.ptr("y"), g.ptr("t"), g.ptr("gup"), g.ptr("coarse"), g.ptr("dy"), int(dy0 is not None),
                               g.ptr("stat"), scal, B, H, W, None)
    torch.cuda.synchronize()
    if expect_rc:
        assert rc < 0, "accepted"
        g.check(untouched=[k for k in ("stat", "dy") if k in items])
        assert all(np.isnan(v) for v in scal)
        return None
    assert rc == 0, (rc, L.xsd_last_error().decode())
    g.check()
    stat = g.t["stat"].view(torch.float64).cpu().numpy().reshape(B, 2)
    return stat, dict(zip(SCAL, scal)), (g.np("dy") if gup is not None else None)


def hold_scale(L, p, t, gup, what, coarse=None, accumulate=False, seed=0, ill_conditioned=False, **kw):
    """forward statistics, scalars and dy of one scale against oracle.ssim_scale; returns (oracle info, device scalars, dy, float64 dy)"""
    B, H, W = p.shape
    sim, cs, back = ol.ssim_scale(p.astype(np.float64), t.astype(np.float64), kw.get("sigma", 2.5), kw.get("k1", 0.01), kw.get("k2", 0.05))
    gup = np.asarray(gup, np.float32).reshape(B, 2)
    ref = back(gup[:, 0].astype(np.float64), gup[:, 1].astype(np.float64))
    info = back.info
    if coarse is not None:
        ref = ref + ol._unpool(coarse.astype(np.float64), (H, W))
    dy0 = None
    if accumulate:
        dy0 = (np.abs(ref).max() * np.random.default_rng(seed).standard_normal(ref.shape)).astype(np.float32)
        ref = ref + dy0
    ref32 = scale_f32(p, t, gup, kw.get("sigma", 2.5), kw.get("k1", 0.01), kw.get("k2", 0.05)) if ill_conditioned else None
    stat, sc, dy = run_scale(L, p, t, gup, coarse, dy0, **kw)
    for b in range(B):
        hold_value("scale value", f"{what} sim[{b}]", stat[b, 0], sim[b])
        hold_value("scale value", f"{what} cs[{b}]", stat[b, 1], cs[b])
        hold_grad("scale dy" + (" sigma 0.3" if ill_conditioned else ""), f"{what} image {b}", dy[b], ref[b], ref32=None if ref32 is None else ref32[b])
    # the four extremes are the inputs' own values; the range and the constants are a handful of fp32 roundings of them (k1, k2 arrive as floats)
    for k in ("pmin", "pmax", "tmin", "tmax"):
        assert np.float32(sc[k]) == np.float32(info[k]), (what, k, sc[k], info[k])
    for k in ("dr", "c1", "c2"):
        hold_value("scale scalars", f"{what} {k}", sc[k], info[k])
        assert abs(sc[k] - info[k]) <= 1e-6 * abs(info[k]), (what, k, sc[k], info[k])
    assert sc["from_p"] == float(info["from_p"]) and sc["nmax"] == info["nmax"] and sc["nmin"] == info["nmin"], (what, sc, info["nmax"], info["nmin"])
    # d loss / d data_range reaches dy only divided by the tie count: held on its own against the larger of itself and the gradient's scale
    err, bar = abs(sc["ddr"] - info["d_dr"]), GRAD_TOL * max(abs(info["d_dr"]), float(np.abs(ref).max()))
    note("scale ddr", what, err, bar)
    assert err <= bar, (what, sc["ddr"], info["d_dr"])
    if not info["from_p"]:
        assert sc["ddr"] == 0.0
    # a forward-only call gives the same statistics bit for bit and leaves the tie counts at 1
    stat2, sc2, none = run_scale(L, p, t, **kw)
    assert none is None and np.array_equal(stat2.view(np.uint64), stat.view(np.uint64)) and sc2["nmax"] == sc2["nmin"] == 1.0 and sc2["ddr"] == 0.0
    return info, sc, dy, ref


def upstream(kind, B, seed):
    rng = np.random.default_rng(seed)
    a, c = 0.5 + rng.random(B), 0.5 + rng.random(B)
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    return {"sim": np.stack([a, 0 * c], 1), "cs": np.stack([0 * a, c], 1), "both": np.stack([a * sign, -c * sign], 1)}[kind]


SCALE_SHAPES = [
    # sigma 2.5, R = 9: one valid pixel; one tile row; exactly one 32 x 32 tile; ragged by one in both directions; 6 blocks in ties / minmax
    (2.5, (1, 19, 19)), (2.5, (2, 19, 51)), (2.5, (2, 50, 50)), (2.5, (1, 51, 83)), (2.5, (3, 83, 49)),
    # sigma 0.3, R = 1
    (0.3, (1, 3, 3)), (0.3, (2, 34, 35)), (0.3, (3, 67, 33)),
    # sigma 3.4, R = 12 = LOSS_RMAX: the tile with its support fills the LDS tile exactly
    (3.4, (1, 25, 25)), (3.4, (2, 56, 57)), (3.4, (3, 89, 55)),
]


@pytest.mark.parametrize("kind", ["sim", "cs", "both"])
@pytest.mark.parametrize("sigma,shape", SCALE_SHAPES, ids=[f"s{s}-{'x'.join(map(str, sh))}" for s, sh in SCALE_SHAPES])
def test_scale_shapes(L, sigma, shape, kind):
    """both images span [0, 1]: the range is the prediction's by the tie rule (python's max keeps the first of two equals)"""
    B, H, W = shape
    p, t = span01(B, H, W, 100 + H + W)
    # sigma 0.3: the gradient's bar is max(project bar, 2 |numpy float32 - float64|) -- measured, not assumed: see scale_f32
    info, sc, _, _ = hold_scale(L, p, t, upstream(kind, B, H), f"{kind} sigma {sigma} {shape}", sigma=sigma, ill_conditioned=sigma == 0.3)
    assert info["from_p"] and info["dr"] == 1.0 and sc["dr"] == 1.0


@pytest.mark.parametrize("kind", ["sim", "cs", "both"])
def test_scale_k1_k2(L, kind):
    p, t = span01(2, 50, 50, 31)
    hold_scale(L, p, t, upstream(kind, 2, 3), f"{kind} k1 0.03 k2 0.1", k1=0.03, k2=0.1)


@pytest.mark.parametrize("shape", [(2, 50, 50), (3, 83, 49)])
@pytest.mark.parametrize("case", ["unique", "two", "row", "target"])
def test_scale_data_range(L, case, shape):
    """whose range it is and how many pixels share its gradient: a unique maximum of 1.5 in the prediction (strictly the prediction's,
    nmax = 1), the same at two pixels, along a whole row, and a target with the wider range (ddr = 0: no term at the extreme pixels)"""
    B, H, W = shape
    p, t = span01(B, H, W, 40 + H)
    where = {"unique": [(B - 1, H // 2, W // 3)], "two": [(0, 3, 5), (B - 1, H - 2, W - 4)], "row": [(B - 1, H // 2, x) for x in range(W)],
             "target": []}[case]
    for i in where:
        p[i] = 1.5
    if case == "target":
        t[0, H // 2, W // 2] = 1.5
    info, sc, dy, ref = hold_scale(L, p, t, upstream("both", B, 5), f"range {case} {shape}")
    assert info["from_p"] == (case != "target") and sc["nmax"] == (len(where) if where else info["nmax"])
    if case == "target":
        hi = p == p.max()
        assert sc["from_p"] == 0.0 and sc["ddr"] == 0.0 and info["d_dr"] == 0.0 and hi.sum() >= 1
    else:
        assert abs(info["d_dr"]) > 10 * GRAD_TOL * np.abs(ref).max() / len(where), "the range term is too small for this case to see it"


@pytest.mark.parametrize("shape", [(2, 51, 83), (1, 19, 21)])
def test_scale_coarse_gradient(L, shape):
    """odd H and W: the pooled scale's gradient reaches 2 x 2 blocks; the last row and column get nothing, as in the oracle's _unpool"""
    B, H, W = shape
    p, t = span01(B, H, W, 50)
    up = upstream("both", B, 6)
    _, _, back = ol.ssim_scale(p.astype(np.float64), t.astype(np.float64))
    scale = np.abs(back(up[:, 0], up[:, 1])).max()                 # a coarse gradient of the scale's own size: neither part hides the other
    coarse = (scale * np.random.default_rng(51).standard_normal((B, H // 2, W // 2))).astype(np.float32)
    _, _, dy, ref = hold_scale(L, p, t, up, f"coarse {shape}", coarse=coarse)
    plain = run_scale(L, p, t, up)[2]
    assert np.array_equal(bits(dy[:, H - 1]), bits(plain[:, H - 1])) and np.array_equal(bits(dy[:, :, W - 1]), bits(plain[:, :, W - 1]))
    assert (dy != plain)[:, :H - 1, :W - 1].mean() > 0.99


def test_scale_accumulates(L):
    p, t = span01(2, 51, 83, 52)
    hold_scale(L, p, t, upstream("both", 2, 7), "accumulate (2, 51, 83)", accumulate=True, seed=53)


def flat_pair():
    p, t = mg.loss_inputs(2, 83, 115, 13)
    p[:, 8:56, 10:58] = 0.0
    t[:, 8:56, 10:58] = 0.0
    p[:, 20:70, 62:110] = 1.0
    return p, t


def test_scale_flat_windows(L):
    """windows that are flat in both images (the zero background of an XMM frame) and windows whose prediction alone is flat: the variance
    clamp's gradient select sits exactly on its threshold there"""
    p, t = flat_pair()
    _, _, back = ol.ssim_scale(p.astype(np.float64), t.astype(np.float64))
    vp, vt = back.info["vp_raw"], back.info["vt_raw"]
    both, nonpos = int(((vp <= 0) & (vt <= 0)).sum()), int((vp <= 0).sum())
    print(f"flat windows: {both} flat in both images, {nonpos} with vp_raw <= 0")
    assert both >= 1000 and nonpos >= 1000
    for kind in ("sim", "cs", "both"):
        hold_scale(L, p, t, upstream(kind, 2, 8), f"flat windows {kind}")


@pytest.mark.parametrize("sigma,R", [(0.3, 1), (2.5, 9), (3.4, 12)])
def test_scale_refuses_what_the_loss_refuses(L, sigma, R):
    """a side of 2R is no window; 2R + 1 is (held to the oracle in test_scale_shapes); sigma 3.6 needs 27 taps"""
    for shape in ((1, 2 * R, 2 * R + 5), (1, 2 * R + 5, 2 * R)):
        p, t = mg.loss_inputs(*shape, 60)
        run_scale(L, p, t, upstream("both", 1, 1), sigma=sigma, expect_rc=-1)
    p, t = mg.loss_inputs(1, 40, 40, 61)
    run_scale(L, p, t, upstream("both", 1, 1), sigma=3.6, expect_rc=-1)
    run_scale(L, p, t, upstream("both", 1, 1), sigma=0.0, expect_rc=-1)


# =====================================================================================================================================
# pooling
# =====================================================================================================================================

@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 19, 45), (1, 38, 39)])
def test_pool2(L, shape):
    """bit for bit the kernel's own fp32 expression, in its order: ((a + b) + c + d) * 0.25; an odd last row / column is dropped"""
    B, H, W = shape
    Ho, Wo = H // 2, W // 2
    p, t = mg.loss_inputs(B, H, W, 70)
    g = Guarded(ro=("p", "t"), p=p, t=t, po=(B, Ho, Wo), to=(B, Ho, Wo))
    rc = L.xsd_loss_test_pool2(g.ptr("p"), g.ptr("t"), g.ptr("po"), g.ptr("to"), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.xsd_last_error().decode())
    g.check()
    for src, name in ((p, "po"), (t, "to")):
        a = src[:, :2 * Ho, :2 * Wo]
        want = (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) * np.float32(0.25)
        assert want.dtype == np.float32 and np.array_equal(bits(g.np(name)), bits(want)), name
        assert np.abs(want - ol._pool(src.astype(np.float64))).max() <= 2.5e-7
    assert L.xsd_loss_test_pool2(g.ptr("p"), g.ptr("t"), g.ptr("po"), g.ptr("to"), B, 1, W, None) < 0


# =====================================================================================================================================
# the whole xsd_loss_eval
# =====================================================================================================================================

def run_eval(L, weights, p, t, want_grad=True, sigma=2.5, k1=0.01, k2=0.05, expect_rc=0):
    """xsd_loss_eval between guard bands -> (out [12], dy or None)"""
    from xmm_superres_denoise.utils import Loss
    f = Loss(weights, 0.0, sigma=sigma, k1=k1, k2=k2)
    B, H, W = p.shape
    g = Guarded(ro=("y", "t"), y=p, t=t, dy=(B, H, W), out=(12,))
    rc = L.xsd_loss_eval(f.h, g.ptr("y"), g.ptr("t"), g.ptr("dy") if want_grad else None, g.ptr("out"), B, H, W, None)
    torch.cuda.synchronize()
    if expect_rc:
        assert rc < 0, f"{p.shape} accepted"
        g.check(untouched=("dy", "out"))
        return None, None
    assert rc == 0, (rc, L.xsd_last_error().decode())
    g.check(untouched=() if want_grad else ("dy",))
    out = g.np("out")
    # zero_kernel / total_kernel: the slots of inactive terms and the reserved ones are 0, whatever the buffer held
    idle = [1 + i for i, k in enumerate(ol.TERMS) if not weights.get(k)] + [9, 10, 11]
    assert not out[idle].any() and not np.isnan(out[idle]).any(), out
    return out, (g.np("dy") if want_grad else None)


def hold_eval(L, weights, p, t, what, family="eval", grad32=None, **kw):
    out, dy = run_eval(L, weights, p, t, **kw)
    total, values, grad = ol.loss_and_grad(p, t, weights, 0.0, kw.get("sigma", 2.5), kw.get("k1", 0.01), kw.get("k2", 0.05))
    for k, v in values.items():
        hold_value(f"{family} value", f"{what} {k}", out[1 + ol.TERMS.index(k)], v)
    hold_value(f"{family} value", f"{what} total", out[0], total)
    hold_grad(f"{family} dy", what, dy, grad, ref32=grad32)
    return out, dy, values, grad


def anti_pair(seed=5):
    _, t = mg.loss_inputs(2, 304, 304, seed)
    return (np.float32(1.0) - t).astype(np.float32), t


def scale_stats(p, t):
    """the float64 statistic of every MS-SSIM scale per image: cs, and sim at the last"""
    p, t, out = p.astype(np.float64), t.astype(np.float64), []
    for s in range(5):
        sim, cs, _ = ol.ssim_scale(p, t)
        out.append(sim if s == 4 else cs)
        p, t = ol._pool(p), ol._pool(t)
    return np.array(out)


def test_eval_anticorrelated_pair_is_exactly_zero(L):
    """p = 1 - t: every scale's statistic is negative, normalize="relu" makes every factor 0: value and gradient vanish exactly"""
    p, t = anti_pair()
    st = scale_stats(p, t)
    print("anti-correlated statistics per scale:", st.round(3).tolist())
    assert (st < 0).all()
    out, dy = run_eval(L, {"ms_ssim": 1.0}, p, t)
    v, g = ol.ms_ssim(p, t)
    assert v == 0.0 and not g.any()
    assert out[5] == 0.0 and out[0] == 0.0 and not dy.any()


def test_eval_half_anticorrelated_batch(L):
    """image 0 anti-correlated, image 1 not: image 0 contributes nothing and receives only the shared data-range term"""
    p, t = anti_pair()
    p[1] = mg.loss_inputs(2, 304, 304, 6)[0][1]
    t[1] = mg.loss_inputs(2, 304, 304, 6)[1][1]
    out, dy, values, grad = hold_eval(L, {"ms_ssim": 1.0}, p, t, "half anti-correlated")
    assert 0.2 < values["ms_ssim"] < 0.5 and (grad[0] != 0).sum() >= 1 and (grad[0] == 0).mean() > 0.9
    assert not dy[0][grad[0] == 0].any(), "image 0 got a gradient where the float64 reference has exactly none"
    hold_grad("eval dy", "half anti-correlated, image 0", dy[0], grad[0])


BIG = (1, 1031, 1019)       # 1,050,589 elements > 4096 * 256: the pointwise gradient's grid-stride loop takes a second pass


@pytest.mark.parametrize("terms", [("l1",), ("poisson",), ("psnr",), ("l1", "poisson", "psnr")], ids=lambda v: "+".join(v))
def test_eval_pointwise_beyond_the_grid_cap(L, terms):
    assert np.prod(BIG) > 4096 * 256
    p, t = mg.loss_inputs(*BIG, 80)
    w = {k: {"l1": 0.3, "poisson": 0.01, "psnr": -0.02}[k] if len(terms) > 1 else 1.0 for k in terms}
    out, dy, _, grad = hold_eval(L, w, p, t, "+".join(terms), family="pointwise")
    if terms == ("l1",):
        inv = np.float32(1.0) / np.float32(p.size)
        d = p - t
        assert (d == 0).sum() > 1000                      # ties at the clip bounds: sign(0) = 0
        assert np.array_equal(bits(dy), bits(np.where(d > 0, inv, np.where(d < 0, -inv, np.float32(0.0)))))


@pytest.mark.parametrize("lo,hi", [(0.2, 0.9), (-0.3, 0.7)])
def test_eval_psnr_data_range(L, lo, hi):
    """torchmetrics' running min / max start at 0: the range of a target in [0.2, 0.9] is 0.9, of one in [-0.3, 0.7] it is 1"""
    p0, t0 = span01(2, 37, 41, 81)
    t = (np.float32(lo) + np.float32(hi - lo) * t0).astype(np.float32)
    p = (t + (p0 - t0) * np.float32(0.5)).astype(np.float32)
    out, dy, values, _ = hold_eval(L, {"psnr": 1.0}, p, t, f"psnr target in [{lo}, {hi}]", family="pointwise")
    d = p.astype(np.float64) - t.astype(np.float64)
    mse = (d * d).mean()
    hold_value("pointwise value", "mse", out[6], mse)
    assert abs(out[6] - mse) <= 1e-6 * mse
    assert np.float32(out[7]) == t.min() and np.float32(out[8]) == t.max()
    dr = max(float(t.max()), 0.0) - min(float(t.min()), 0.0)
    assert abs(dr - (hi - min(lo, 0.0))) < 1e-6 and abs(values["psnr"] - 10 * np.log10(dr * dr / mse)) < 1e-9
    if lo > 0:      # max - min would be 0.7: 2.2 dB less
        assert values["psnr"] - 10 * np.log10((float(t.max()) - float(t.min())) ** 2 / mse) > 2.0


def test_eval_sparse_pair(L):
    """p == 0 on most pixels where t > 0 (a sparse prediction of a source field): the Poisson term's log(1e-8) and 1 / 1e-8 everywhere,
    zero background windows in the SSIM terms; every term alone (its own gradient scale) and all five together"""
    rng = np.random.default_rng(82)
    _, t = mg.loss_inputs(2, 304, 304, 83)
    p = np.where(rng.random(t.shape) < 0.1, t, np.float32(0.0)).astype(np.float32)
    assert ((p == 0) & (t > 0)).mean() > 0.8
    for term in ol.TERMS:
        hold_eval(L, {term: 1.0}, p, t, f"sparse {term}", family="sparse")
    hold_eval(L, {"l1": 0.3, "poisson": 0.01, "psnr": -0.02, "ssim": -0.4, "ms_ssim": -0.5}, p, t, "sparse, five terms", family="sparse")


def test_eval_plain_ssim_beyond_256_images(L):
    """combine_kernel's loop over the images takes a second pass"""
    p, t = span01(300, 19, 21, 84)
    out, dy, _, grad = hold_eval(L, {"ssim": 1.0}, p, t, "ssim (300, 19, 21)")
    for b in (0, 255, 256, 299):
        hold_grad("eval dy", f"ssim (300, 19, 21) image {b}", dy[b], grad[b])


@pytest.mark.parametrize("term", ol.TERMS)
def test_eval_nan_pixel_makes_the_total_nan(L, term):
    p, t = mg.loss_inputs(1, 304, 304, 85)
    p[0, 100, 100] = np.nan
    out, _ = run_eval(L, {term: 1.0}, p, t)
    v = ol._FUNCS[term](p, t, want_grad=False)[0]
    assert np.isnan(v)
    assert np.isnan(out[0]) and np.isnan(out[1 + ol.TERMS.index(term)]), (term, out[:6])


def both_ways(h, w):
    return [(1, h, w), (1, w, h)]


@pytest.mark.parametrize("sigma,R", [(0.3, 1), (2.5, 9), (3.4, 12)])
def test_eval_ssim_bounds(L, sigma, R):
    """ssim: a side of 2R is refused, 2R + 1 accepted and right, on H and on W"""
    for shape in both_ways(2 * R, 2 * R + 5):
        run_eval(L, {"ssim": 1.0}, *mg.loss_inputs(*shape, 90), sigma=sigma, expect_rc=-1)
    for shape in both_ways(2 * R + 1, 2 * R + 5):
        p, t = span01(*shape, 91)
        g32 = scale_f32(p, t, [[1.0, 0.0]], sigma) if sigma == 0.3 else None      # sigma 0.3: the ill-conditioned window, as in test_scale_shapes
        hold_eval(L, {"ssim": 1.0}, p, t, f"ssim sigma {sigma} {shape}", family="bounds" + (" sigma 0.3" if sigma == 0.3 else ""), grad32=g32, sigma=sigma)


def test_eval_sigma_bound(L):
    """sigma 3.6 needs 27 taps (refused); sigma 3.5 is R = 12 too, with other taps than 3.4"""
    shape = (1, 30, 31)
    run_eval(L, {"ssim": 1.0}, *mg.loss_inputs(*shape, 92), sigma=3.6, expect_rc=-1)
    hold_eval(L, {"ssim": 1.0}, *span01(*shape, 92), "ssim sigma 3.5", family="bounds", sigma=3.5)


@pytest.mark.parametrize("sigma,refused", [(2.5, 303), (0.3, 207), (3.4, 399)])
def test_eval_ms_ssim_bounds(L, sigma, refused):
    """ms_ssim: 304 is the first size whose coarsest scale holds the 19-tap window; with 3 taps torchmetrics' own kernel_size rule binds
    (208); with 25 taps the coarsest scale needs 25 pixels (400)"""
    for shape in both_ways(refused, refused + 9):
        run_eval(L, {"ms_ssim": 1.0}, *mg.loss_inputs(*shape, 93), sigma=sigma, expect_rc=-1)
        if sigma == 0.3:      # torchmetrics' own rule (kernel_size), which the oracle restates; the window rule at the coarsest scale is this project's
            with pytest.raises(ValueError):
                ol.ms_ssim(*mg.loss_inputs(*shape, 93), sigma=sigma)
    for shape in both_ways(refused + 1, refused + 9):
        hold_eval(L, {"ms_ssim": 1.0}, *mg.loss_inputs(*shape, 94), f"ms_ssim sigma {sigma} {shape}", family="bounds", sigma=sigma)
