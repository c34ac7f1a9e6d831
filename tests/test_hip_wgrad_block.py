"""A dense block's weight gradients as the shipped plan launches them, through xsd_test_wgrad_block: ONE pair-list launch of wgrad_s3x /
wgrad_h2x over the fifteen (x_j, G_n) pairs (npairs = 15) plus ONE wgrad_reduce_multi launch for the five convs.  The launch and the
reductions are filled by the function the plan calls (wgrad_block_fill, csrc/xsd_engine.hip); the hook fills both partial-sum buffers
with 0xFF bytes first, so a panel or a bias row that no workgroup writes arrives in dw / db as NaN.

Reference: float64 autograd, L_n = sum(conv2d(cat(x_0 .. x_n), w_n, b_n, padding=1) * G_{n+1}) at w = 0; conv 5 times float32(gscale).
Bar: max|got - ref| <= 5e-5 * max|ref| (TOL of test_hip_wgrad_views.py) per conv for dw and db AND per (j, n) block of dw, each block
against its own maximum: every block's products are formed with its own operand scales, and a large block must not hide a small one.
The five convs' dw / db lie in one flat NaN-prefilled buffer with gaps between them; whatever no conv owns must stay NaN."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_wgrad_views import GUARD, TOL, assert_close, host, run_wgrad, to_plane
from util_hip import guarded_planes

pytestmark = pytest.mark.gpu

GAP = 96      # NaN floats between two regions of the flat buffer
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 19, 45), (3, 40, 100)]      # 1 / 3 / 12 (h2x: 32 x 8 tiles), 20 (s3x: 32 x 4) / 60, 120 tiles
NPARTS = [8, 9, 16, 17, 80, 81]
WORST = {}    # mode -> {what: worst err / bar}: printed by the last test


def layout():
    """(w_off[5], b_off[5], total): conv n + 1 owns [32][32 (n + 1)][3][3] at w_off[n] and [32] at b_off[n], GAP NaNs around each"""
    w_off, b_off, off = [], [], GUARD
    for n in range(5):
        w_off.append(off)
        off += 32 * 32 * (n + 1) * 9 + GAP
        b_off.append(off)
        off += 32 + GAP
    return w_off, b_off, off - GAP + GUARD


W_OFF, B_OFF, TOTAL = layout()


@pytest.fixture(scope="module", params=["bf16x6", "f16x3"])
def eng(request):
    return fresh_engine(request.param)


def fresh_engine(mode):
    from xmm_superres_denoise.engine import Engine
    e = Engine("dn", 1, 1, 32, 1)
    e.set_math(mode)
    return e


def plan_nparts(ncu):
    """block_parts_per_xcd's rule (csrc/xsd_engine.hip): m = CUs / 120 parts per XCD, at most 10; one more part when >= 16 CUs are left"""
    m = min(ncu // 120, 10)
    return 8 * m + (1 if ncu - 120 * m >= 16 else 0)


_DATA, _REF = {}, {}


def data(shape, seed=0):
    """xs = x_0 .. x_4, gs = G_1 .. G_5: five [B, 32, H, W] float32 arrays each (shared between tests: never modified)"""
    if (shape, seed) not in _DATA:
        rng = np.random.default_rng(1000 * seed + shape[1] * 101 + shape[2])
        B, H, W = shape
        _DATA[(shape, seed)] = ([rng.normal(size=(B, 32, H, W)).astype(np.float32) for _ in range(5)],
                                [rng.normal(size=(B, 32, H, W)).astype(np.float32) for _ in range(5)])
    return _DATA[(shape, seed)]


def reference(xs, gs, gscale=1.0, key=None):
    """[(dw_n, db_n)] in float64; cached under `key` (computed once per data set, shared, never modified)"""
    if key is not None and key in _REF:
        return _REF[key]
    out = []
    for n in range(5):
        xt = torch.from_numpy(np.concatenate(xs[:n + 1], axis=1)).double()
        w = torch.zeros((32, 32 * (n + 1), 3, 3), dtype=torch.float64, requires_grad=True)
        b = torch.zeros((32,), dtype=torch.float64, requires_grad=True)
        (F.conv2d(xt, w, b, padding=1) * torch.from_numpy(gs[n]).double()).sum().backward()
        s = float(np.float32(gscale)) if n == 4 else 1.0
        out.append((w.grad.numpy() * s, b.grad.numpy() * s))
    if key is not None:
        _REF[key] = out
    return out


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_block(eng, xs, gs, nparts=0, gscale=1.0, separate=0, expect_rc=0, null_plane=None):
    """One xsd_test_wgrad_block call on guarded copies of the ten planes.  Returns ([(dw_n, db_n)] as numpy, the nparts the hook reports).
    Asserts: the return code, the planes and their guard bands untouched, everything outside the five convs' regions still NaN
    (on a refusal: the whole buffer)."""
    B, _, H, W = xs[0].shape
    x_orig, g_orig = [to_plane(a) for a in xs], [to_plane(a) for a in gs]
    xd, chk_x = guarded_planes(5, B, H, W, x_orig)
    gd, chk_g = guarded_planes(5, B, H, W, g_orig)
    buf = torch.full((TOTAL,), float("nan"), device="cuda")
    ptrs = [t.data_ptr() for t in xd] + [t.data_ptr() for t in gd]
    if null_plane is not None:
        ptrs[null_plane] = None
    xp, gp = (ctypes.c_void_p * 5)(*ptrs[:5]), (ctypes.c_void_p * 5)(*ptrs[5:])
    used = ctypes.c_int(-1)
    rc = eng.L.xsd_test_wgrad_block(eng.h, xp, gp, gscale, buf.data_ptr(), (ctypes.c_int64 * 5)(*W_OFF), (ctypes.c_int64 * 5)(*B_OFF),
                                    nparts, separate, ctypes.byref(used), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, eng.L.xsd_last_error().decode())
    chk_x()
    chk_g()
    for a, o in zip(list(xd) + list(gd), x_orig + g_orig):
        assert same_bits(a, o), "an operand plane was modified"
    flat = buf.cpu().numpy()
    owned = np.zeros(TOTAL, bool)
    res = []
    for n in range(5):
        nw = 32 * 32 * (n + 1) * 9
        owned[W_OFF[n]:W_OFF[n] + nw] = True
        owned[B_OFF[n]:B_OFF[n] + 32] = True
        res.append((flat[W_OFF[n]:W_OFF[n] + nw].reshape(32, 32 * (n + 1), 3, 3).copy(), flat[B_OFF[n]:B_OFF[n] + 32].copy()))
    if rc != 0:
        assert np.isnan(flat).all(), "a refused call wrote to the gradient buffer"
        assert used.value == -1
        return None, None
    assert np.isnan(flat[~owned]).all(), "a store between or around the five convs' regions"
    return res, used.value


def note(eng, what, ratio):
    w = WORST.setdefault(eng.get_math(), {})
    w[what] = max(w.get(what, 0.0), ratio)


def ratio_of(got, ref):
    bar = TOL * float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    return (err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))), err, bar


def check_against(eng, res, ref, what, convs=range(5), blocks=None):
    """the bar per conv (dw, db) and per (j, n) block of dw; every figure printed before it is asserted"""
    lines, bad = [], []
    for n in convs:
        (dw, db), (dw_ref, db_ref) = res[n], ref[n]
        assert np.isfinite(dw).all() and np.isfinite(db).all(), f"{what}: conv {n + 1} has a non-finite entry (nobody wrote it, or a product overflowed)"
        items = [(f"conv{n + 1} dw", dw, dw_ref, "dw per conv"), (f"conv{n + 1} db", db, db_ref, "db per conv")]
        items += [(f"block (j={j}, n={n})", dw[:, 32 * j:32 * j + 32], dw_ref[:, 32 * j:32 * j + 32], "dw per block")
                  for j in range(n + 1) if blocks is None or (j, n) in blocks]
        for name, g, r, klass in items:
            ratio, err, bar = ratio_of(g, r)
            note(eng, klass, ratio)
            lines.append(f"{what} {name}: err {err:.3e} bar {bar:.3e} err/bar {ratio:.3f}")
            if not ratio <= 1.0:
                bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


def bits_equal(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for (aw, ab), (bw, bb) in zip(a, b) for x, y in ((aw, bw), (ab, bb)))


@pytest.mark.parametrize("nparts", [0] + NPARTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_launch_against_float64(eng, shape, nparts):
    xs, gs = data(shape)
    res, used = run_block(eng, xs, gs, nparts=nparts, gscale=0.2)
    if nparts == 0:
        ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        assert used == plan_nparts(ncu), (used, ncu)
        assert used % 8 in (0, 1) and 1 <= used // 8 <= 10
        if ncu == 256:
            assert used == 17
    else:
        assert used == nparts
    check_against(eng, res, reference(xs, gs, 0.2, key=(shape, 0, 0.2)), f"{shape} nparts {used}")
    if shape == (1, 1, 1):      # one pixel: only the centre tap sees it
        for n in range(5):
            off_centre = res[n][0].reshape(32, -1, 9)[:, :, [0, 1, 2, 3, 5, 6, 7, 8]]
            assert not off_centre.any(), f"conv {n + 1}: a tap other than the centre is not exactly 0"


@pytest.mark.parametrize("nparts", [16, 17])
def test_one_hot_x_plane(eng, nparts):
    """x_2 alone is non-zero: every block with j != 2 is exactly zero, the j = 2 blocks of convs 3, 4 and 5 meet the bar"""
    shape = (2, 19, 45)
    xs, gs = data(shape)
    xs = [a if j == 2 else np.zeros_like(a) for j, a in enumerate(xs)]
    res, _ = run_block(eng, xs, gs, nparts=nparts)
    for n in range(5):
        for j in range(n + 1):
            if j != 2:
                assert not res[n][0][:, 32 * j:32 * j + 32].any(), f"block (j={j}, n={n}) is not exactly zero"
    ref = reference(xs, gs, key=(shape, "x2"))
    check_against(eng, res, ref, f"x_2 only, nparts {nparts}", convs=(2, 3, 4), blocks={(2, 2), (2, 3), (2, 4)})
    for n in range(5):      # db does not depend on x
        r, err, bar = ratio_of(res[n][1], ref[n][1])
        assert r <= 1.0, (n, err, bar)


@pytest.mark.parametrize("nparts", [16, 17])
def test_one_hot_g_plane(eng, nparts):
    """G_4 alone is non-zero: only conv 4's dw and db may be non-zero"""
    shape = (2, 19, 45)
    xs, gs = data(shape)
    gs = [a if n == 3 else np.zeros_like(a) for n, a in enumerate(gs)]
    res, _ = run_block(eng, xs, gs, nparts=nparts)
    for n in range(5):
        if n != 3:
            assert not res[n][0].any() and not res[n][1].any(), f"conv {n + 1} is not exactly zero"
    check_against(eng, res, reference(xs, gs, key=(shape, "g4")), f"G_4 only, nparts {nparts}", convs=(3,))


FX = [1.0, 2.0 ** 10, 1.0, 2.0 ** -9, 1.0]
FG = [1.0, 2.0 ** -12, 1.0, 1.0, 2.0 ** 8]


@pytest.mark.parametrize("nparts", [16, 17])
def test_planes_of_different_magnitude(eng, nparts):
    """x_1 * 2^10, x_3 * 2^-9, G_2 * 2^-12, G_5 * 2^8: the per-block bar, and -- every factor being a power of two, every split, product
    and sum of both modes scaling exactly (f16x3: the operand scale 2^k follows the plane's max |x| exactly; no value leaves the normal
    range) -- each block equal to the unscaled run's block times its two factors, bit for bit"""
    shape = (2, 19, 45)
    xs, gs = data(shape)
    xs2 = [(a * np.float32(f)).astype(np.float32) for a, f in zip(xs, FX)]
    gs2 = [(a * np.float32(f)).astype(np.float32) for a, f in zip(gs, FG)]
    res, _ = run_block(eng, xs2, gs2, nparts=nparts)
    check_against(eng, res, reference(xs2, gs2, key=(shape, "mag")), f"scaled planes, nparts {nparts}")
    base, _ = run_block(eng, xs, gs, nparts=nparts)
    for n in range(5):
        assert np.array_equal(res[n][1], base[n][1] * np.float32(FG[n])), f"db of conv {n + 1} is not the unscaled db times 2^k"
        for j in range(n + 1):
            sl = slice(32 * j, 32 * j + 32)
            assert np.array_equal(res[n][0][:, sl], base[n][0][:, sl] * np.float32(FX[j] * FG[n])), f"block (j={j}, n={n}) is not the unscaled block times 2^k"


def test_no_stale_partial_sums(eng):
    """(3, 40, 100) at 81 parts, then (1, 1, 1) at 8: the second result is a fresh engine's, bit for bit"""
    big, small = data((3, 40, 100)), data((1, 1, 1))
    run_block(eng, *big, nparts=81)
    second, _ = run_block(eng, *small, nparts=8)
    first, _ = run_block(fresh_engine(eng.get_math()), *small, nparts=8)
    assert bits_equal(second, first)
    check_against(eng, second, reference(*small, key=((1, 1, 1), 0, 1.0)), "(1, 1, 1) after (3, 40, 100)")


@pytest.mark.parametrize("shape,nparts", [((3, 5, 7), 9), ((2, 19, 45), 17), ((3, 40, 100), 80)])
def test_one_reduce_launch_is_five_and_runs_repeat(eng, shape, nparts):
    xs, gs = data(shape)
    a, _ = run_block(eng, xs, gs, nparts=nparts, gscale=0.2)
    b, _ = run_block(eng, xs, gs, nparts=nparts, gscale=0.2)
    c, _ = run_block(eng, xs, gs, nparts=nparts, gscale=0.2, separate=1)
    assert bits_equal(a, b), "two runs differ"
    assert bits_equal(a, c), "five reduce launches differ from the one wgrad_reduce_multi launch"
    check_against(eng, c, reference(xs, gs, 0.2, key=(shape, 0, 0.2)), f"{shape} separate reduces")


def test_gscale_scales_conv5_only(eng):
    shape = (2, 19, 45)
    xs, gs = data(shape)
    one, _ = run_block(eng, xs, gs, nparts=17, gscale=1.0)
    fifth, _ = run_block(eng, xs, gs, nparts=17, gscale=0.2)
    assert bits_equal(one[:4], fifth[:4]), "gscale reached one of convs 1 .. 4"
    check_against(eng, one, reference(xs, gs, 1.0, key=(shape, 0, 1.0)), "gscale 1")
    check_against(eng, fifth, reference(xs, gs, 0.2, key=(shape, 0, 0.2)), "gscale 0.2")
    # the reduction multiplies its double sum by the float gscale before the one rounding to float
    assert not np.array_equal(one[4][0], fifth[4][0]) and not np.array_equal(one[4][1], fifth[4][1])


@pytest.mark.parametrize("nparts", [16, 17])
@pytest.mark.parametrize("shape", [(2, 19, 45), (3, 40, 100)], ids=lambda s: "x".join(map(str, s)))
def test_against_the_rectangle_form(eng, shape, nparts):
    """conv n + 1 through xsd_test_wgrad_ex (x_0 .. x_n against G_{n+1}, the per-G launch of the plan): another cut of the same sums,
    2e-6 of the maximum as in test_hip_network.py::test_block_weight_gradient_launch_equals_one_launch_per_g.  (At (2, 19, 45) no part of
    either form holds more than one of wgrad_h2x's 12 tiles and the reduction's double sums are exact: f16x3 agrees bit for bit there.)"""
    xs, gs = data(shape)
    res, _ = run_block(eng, xs, gs, nparts=nparts)
    for n in range(5):
        dw, db = host(*run_wgrad(eng, np.concatenate(xs[:n + 1], axis=1), gs[n], 32 * (n + 1), 32), 32 * (n + 1), 32)
        for name, a, b in (("dw", res[n][0], dw), ("db", res[n][1], db)):
            d, mx = float(np.abs(a - b).max()), float(np.abs(b).max())
            print(f"conv {n + 1} {name}: |block - rectangle| {d:.3e}  2e-6 max {2e-6 * mx:.3e}")
            assert d <= 2e-6 * mx, (n, name, d, mx)


def test_a_nan_in_g3_reaches_conv3_only(eng):
    shape = (2, 19, 45)
    xs, gs = data(shape)
    gs = [a.copy() if n == 2 else a for n, a in enumerate(gs)]
    c = 11
    gs[2][1, c, 7, 20] = np.nan
    res, _ = run_block(eng, xs, gs, nparts=17)
    ref = reference(*data(shape), key=(shape, 0, 1.0))
    check_against(eng, res, ref, "NaN in G_3", convs=(0, 1, 3, 4))
    dw, db = res[2]
    # G_3[b, c, y, x] multiplies x[., y + ky - 1, x + kx - 1] into row c of dw for all nine taps (an interior pixel), and is a term of db[c]
    assert np.isnan(dw[c]).all() and np.isnan(db[c])
    rows = np.arange(32) != c
    assert np.isfinite(dw[rows]).all() and np.isfinite(db[rows]).all(), "the NaN reached another output channel"
    for name, g, r in (("dw", dw[rows], ref[2][0][rows]), ("db", db[rows], ref[2][1][rows])):
        ratio, err, bar = ratio_of(g, r)
        print(f"conv3 {name}, rows other than {c}: err {err:.3e} bar {bar:.3e}")
        assert ratio <= 1.0, (name, err, bar)


@pytest.mark.parametrize("nparts", [-8, 1, 7, 10, 15, 18, 88, 89, 256])
def test_an_nparts_of_another_form_is_refused(eng, nparts):
    run_block(eng, *data((3, 5, 7)), nparts=nparts, expect_rc=-1)


@pytest.mark.parametrize("which", [0, 4, 5, 9])
def test_a_null_plane_is_refused(eng, which):
    run_block(eng, *data((3, 5, 7)), nparts=16, expect_rc=-1, null_plane=which)


def test_fp32_mode_and_generic_width_engines_are_refused():
    from xmm_superres_denoise.engine import Engine
    run_block(fresh_engine("fp32"), *data((3, 5, 7)), nparts=16, expect_rc=-1)
    run_block(Engine("dn", 1, 1, 264, 1), *data((3, 5, 7)), nparts=16, expect_rc=-1)


def test_worst_ratios_table():
    """prints what the tests above measured (run alone it has nothing to print)"""
    for mode, w in sorted(WORST.items()):
        print(mode, "  ".join(f"{k}: worst err/bar {v:.3f}" for k, v in sorted(w.items())))
        assert all(v <= 1.0 for v in w.values())
