"""The RRDB weight-gradient kernels one by one (wgrad_mfma / wgrad_s3x / wgrad_h2x + the fixed-order reduction) through
xsd_test_wgrad_ex: the n_in x n_g rectangle (in the split modes 2 and 4 pairs run as ONE round over nparts / pairs parts), the
pixel-shuffled G views with the shuffled reduction, the reduction's j0 / n0 / plane offsets and its scale.

Reference: float64 autograd through torch.nn.functional.conv2d (and pixel_shuffle where shuffled), loss = sum(y * G).
Bar: max|got - ref| <= 5e-5 * max|ref| for dw and db, as test_hip_kernels.py::test_conv3x3_backward.  dw and db are pre-filled with
NaN between NaN guard bands: what a launch does not own must stay NaN."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util_hip import guarded_planes

pytestmark = pytest.mark.gpu

TOL = 5e-5
GUARD = 4096


@pytest.fixture(scope="module", params=["fp32", "bf16x6", "f16x3"])
def eng(request):
    from xmm_superres_denoise.engine import Engine
    e = Engine("dn", 1, 1, 32, 1)
    e.set_math(request.param)
    return e


def to_plane(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()


def run_wgrad(eng, x, g, cin_total, cout_total, shuffle_g=False, shuffle=0, plane=0, j0=0, n0=0, scale=1.0, dw=None, db=None, expect_rc=0):
    """x: [B, 32 n_in, H, W]; g: [B, 32 n_g, H, W], or with shuffle_g ONE high-resolution plane [B, 32, 2H, 2W] (n_g = 4).
    Returns (dw, db) as numpy, NaN where the launch wrote nothing; pass the previous (dw, db) device buffers back in to go on filling them."""
    B, _, H, W = x.shape
    n_in, n_g = x.shape[1] // 32, (4 if shuffle_g else g.shape[1] // 32)
    x_orig = [to_plane(x[:, 32 * i:32 * i + 32]) for i in range(n_in)]
    xs, chk_x = guarded_planes(n_in, B, H, W, x_orig)
    if shuffle_g:
        g_orig = [to_plane(g)]
        gs, chk_g = guarded_planes(1, B, 2 * H, 2 * W, g_orig)
    else:
        g_orig = [to_plane(g[:, 32 * i:32 * i + 32]) for i in range(n_g)]
        gs, chk_g = guarded_planes(n_g, B, H, W, g_orig)
    nw = cout_total * cin_total * 9
    if dw is None:
        dw = torch.full((2 * GUARD + nw,), float("nan"), device="cuda")
        db = torch.full((2 * GUARD + cout_total,), float("nan"), device="cuda")
    xp = (ctypes.c_void_p * n_in)(*[t.data_ptr() for t in xs])
    gp = (ctypes.c_void_p * len(gs))(*[t.data_ptr() for t in gs])
    rc = eng.L.xsd_test_wgrad_ex(eng.h, xp, n_in, gp, n_g, int(shuffle_g), scale, shuffle, plane, j0, n0, cin_total, cout_total,
                                 dw[GUARD:].data_ptr(), db[GUARD:].data_ptr(), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, eng.L.xsd_last_error().decode())
    chk_x()
    chk_g()
    for a, o in zip(list(xs) + list(gs), x_orig + g_orig):
        assert torch.equal(a, o), "an operand plane was modified"
    for buf, n in ((dw, nw), (db, cout_total)):
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "a store outside dw / db"
    return dw, db


def host(dw, db, cin_total, cout_total):
    return (dw[GUARD:GUARD + cout_total * cin_total * 9].cpu().numpy().reshape(cout_total, cin_total, 3, 3),
            db[GUARD:GUARD + cout_total].cpu().numpy())


def reference(x, g, cout, shuffled_plane=None):
    """dL/dw, dL/db of L = sum(conv2d(x, w, b) * g) in float64; with shuffled_plane = p, L = sum(pixel_shuffle(conv2d(x, w, b), 2)[:, 32p : 32p + 32] * g_hr)"""
    xt = torch.from_numpy(x).double()
    w = torch.zeros((cout, x.shape[1], 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xt, w, b, padding=1)
    if shuffled_plane is not None:
        y = F.pixel_shuffle(y, 2)[:, 32 * shuffled_plane:32 * shuffled_plane + 32]
    (y * torch.from_numpy(g).double()).sum().backward()
    return w.grad.numpy(), b.grad.numpy()


def assert_close(got, ref, what):
    err, bar = float(np.abs(got - ref).max()), TOL * float(np.abs(ref).max())
    print(f"{what}: max|got - ref| {err:.3e}  bar {bar:.3e}")
    assert np.isfinite(got).all(), f"{what}: an entry the launch owns was not written"
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def make(rng, B, H, W, n_in, n_g):
    return rng.normal(size=(B, 32 * n_in, H, W)).astype(np.float32), rng.normal(size=(B, 32 * n_g, H, W)).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 19, 45), (3, 5, 7)])
@pytest.mark.parametrize("n_in,n_g", [(1, 2), (2, 2), (1, 4), (4, 1), (5, 1)])
def test_rectangles(eng, n_in, n_g, shape):
    """(1, 2), (2, 2) and (1, 4) take the nparts / pairs single-round form in the split modes"""
    B, H, W = shape
    x, g = make(np.random.default_rng(10 * n_in + n_g), B, H, W, n_in, n_g)
    dw, db = host(*run_wgrad(eng, x, g, 32 * n_in, 32 * n_g), 32 * n_in, 32 * n_g)
    dw_ref, db_ref = reference(x, g, 32 * n_g)
    assert_close(dw, dw_ref, f"dw {n_in} x {n_g}")
    assert_close(db, db_ref, f"db {n_in} x {n_g}")


@pytest.mark.parametrize("shape", [(2, 19, 45), (3, 5, 7)])
@pytest.mark.parametrize("plane,cout_total", [(0, 128), (0, 256), (1, 256)])
def test_shuffled_g(eng, plane, cout_total, shape):
    """one high-resolution G plane read as its four sub-pixel views, reduced with shuffle = 1: dw rows land at oc = 4 (32 plane + co) + n,
    the rows of the other plane of a two-plane high-resolution tensor stay NaN"""
    B, H, W = shape
    rng = np.random.default_rng(50 + plane + cout_total)
    x = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    ghr = rng.normal(size=(B, 32, 2 * H, 2 * W)).astype(np.float32)
    dw, db = host(*run_wgrad(eng, x, ghr, 32, cout_total, shuffle_g=True, shuffle=1, plane=plane), 32, cout_total)
    dw_ref, db_ref = reference(x, ghr, cout_total, shuffled_plane=plane)
    own = slice(128 * plane, 128 * plane + 128)
    assert_close(dw[own], dw_ref[own], "dw shuffled")
    assert_close(db[own], db_ref[own], "db shuffled")
    other = np.ones(cout_total, bool)
    other[own] = False
    assert np.isnan(dw[other]).all() and np.isnan(db[other]).all(), "rows of the other plane were written"
    assert not dw_ref[other].any()


@pytest.mark.parametrize("split", ["n0", "j0"])
def test_two_launches_fill_a_64_to_64_conv(eng, split):
    """each launch writes only its own block of dw (and its own part of db): by output chunk (n0) or by input plane (j0)"""
    B, H, W = 2, 19, 45
    x, g = make(np.random.default_rng(64), B, H, W, 2, 2)
    dw_ref, db_ref = reference(x, g, 64)
    sl = lambda k: slice(32 * k, 32 * k + 32)
    if split == "n0":
        bufs = run_wgrad(eng, x, g[:, sl(1)], 64, 64, n0=1)
        dw, db = host(*bufs, 64, 64)
        assert np.isnan(dw[sl(0)]).all() and np.isnan(db[sl(0)]).all(), "the launch for chunk 1 wrote chunk 0"
        assert_close(dw[sl(1)], dw_ref[sl(1)], "dw chunk 1")
        assert_close(db[sl(1)], db_ref[sl(1)], "db chunk 1")
        bufs = run_wgrad(eng, x, g[:, sl(0)], 64, 64, n0=0, dw=bufs[0], db=bufs[1])
    else:
        bufs = run_wgrad(eng, x[:, sl(1)], g, 64, 64, j0=1)
        dw, db = host(*bufs, 64, 64)
        assert np.isnan(dw[:, sl(0)]).all(), "the launch for input plane 1 wrote input plane 0"
        assert_close(dw[:, sl(1)], dw_ref[:, sl(1)], "dw plane 1")
        bufs = run_wgrad(eng, x[:, sl(0)], g, 64, 64, j0=0, dw=bufs[0], db=bufs[1])
    dw, db = host(*bufs, 64, 64)
    assert_close(dw, dw_ref, "dw 64 -> 64")
    assert_close(db, db_ref, "db 64 -> 64")


@pytest.mark.parametrize("n_in,n_g", [(2, 2), (5, 1)])
def test_scale(eng, n_in, n_g):
    B, H, W = 2, 19, 45
    x, g = make(np.random.default_rng(20 + n_in), B, H, W, n_in, n_g)
    dw, db = host(*run_wgrad(eng, x, g, 32 * n_in, 32 * n_g, scale=0.2), 32 * n_in, 32 * n_g)
    dw_ref, db_ref = reference(x, g, 32 * n_g)
    s = float(np.float32(0.2))
    assert_close(dw, s * dw_ref, "dw x 0.2")
    assert_close(db, s * db_ref, "db x 0.2")


def test_shuffled_weight_gradient_is_bitwise_reproducible(eng):
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(3)
    x = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    ghr = rng.normal(size=(B, 32, 2 * H, 2 * W)).astype(np.float32)
    res = [host(*run_wgrad(eng, x, ghr, 32, 256, shuffle_g=True, shuffle=1, plane=1), 32, 256) for _ in range(2)]
    own = slice(128, 256)
    assert np.array_equal(res[0][0][own], res[1][0][own]) and np.array_equal(res[0][1][own], res[1][1][own])


@pytest.mark.parametrize("kw", [dict(n_in=6, n_g=1), dict(n_in=1, n_g=5), dict(n_in=2, n_g=3),dict(n_in=1, n_g=2, cout_total=32), dict(n_in=2, n_g=1, cin_total=32),
                                dict(n_in=1, n_g=4, shuffle=1, plane=1, cout_total=128), dict(n_in=1, n_g=2, shuffle=1)])
def test_what_the_partial_sums_do_not_hold_is_refused(eng, kw):
    """XSD_ERR_ARG before anything is launched: more planes than wg_partial holds, a block outside [cout_total][cin_total]"""
    n_in, n_g = kw["n_in"], kw["n_g"]
    B, H, W = 1, 8, 32
    planes = [torch.zeros((B, H, W, 32), device="cuda") for _ in range(n_in + n_g)]
    xp = (ctypes.c_void_p * n_in)(*[t.data_ptr() for t in planes[:n_in]])
    gp = (ctypes.c_void_p * n_g)(*[t.data_ptr() for t in planes[n_in:]])
    cin, cout = kw.get("cin_total", 32 * n_in), kw.get("cout_total", 32 * n_g)
    dw = torch.full((max(cout, 256) * max(cin, 192) * 9,), float("nan"), device="cuda")
    db = torch.full((256,), float("nan"), device="cuda")
    rc = eng.L.xsd_test_wgrad_ex(eng.h, xp, n_in, gp, n_g, 0, 1.0, kw.get("shuffle", 0), kw.get("plane", 0), 0, 0, cin, cout,
                                 dw.data_ptr(), db.data_ptr(), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == -1, rc
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())
