"""The input-transform kernels one by one (csrc/aux_kernels.hip: mask_pad_normalize_kernel, compose_batch_kernel, normalize_kernel,
upsample_nearest_kernel) at the inputs tests/test_hip_transforms.py and tests/test_hip_dataset.py do not reach: NaN / inf / -0.0 words,
both clamp bounds, a crop fused with the upsample, big-endian float32 words, extra planes on the float path, the second pass of the
grid-stride loops, the 128-sample chunk boundary of xsd_compose_batch, guard bands around every output, inputs that come back unchanged.
The references are plain numpy written from the reference project's formulas (data/tools.py:103-126 reshape_img_to_res,
transforms/normalize.py, transforms/imageupsample.py, data/dataset.py:24-49): fp32 numpy where the engine is exact (geometry, linear
stretch, ImageUpsample), float64 with the reference's own fp32 torch evaluation as the yardstick for asinh / log."""
import ctypes

import numpy as np
import pytest
import torch

from test_hip_sw_kernels import _assert_within_2x_of_fp32
from util_hip import Guarded

pytestmark = pytest.mark.gpu

f32 = np.float32
STRETCH = {"linear": 0, "sqrt": 1, "asinh": 2, "log": 3}
ERR_ARG = -1
INT_SPECIALS = np.array([-5, -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1], np.int64)       # negative counts, both ends, the conversion's rounding


def _lib():
    from xmm_superres_denoise.engine import _lib as m
    return m.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def same(got, want, what):
    """bit for bit, NaNs by position only (a NaN's payload and sign are not specified)"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), f"{what}: NaNs at {np.argwhere(ng != nw)[:4].tolist()} differ"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nw
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {i}: got {got[i]!r}, expected {want[i]!r}")


# ---- sample data ---------------------------------------------------------------------------------------------------------------------
def make_planes(rng, n, B, Hin, Win, is_int32, seed):
    """n planes [B][Hin][Win] of native values: int32 counts (with the special values dealt round) or float32 (a NaN and a -0.0 in the first)"""
    out = []
    for k in range(n):
        if is_int32:
            v = rng.integers(-2 ** 26, 2 ** 26, size=(B, Hin, Win), dtype=np.int64)
            flat = v.reshape(-1)
            m = min(flat.size, 4)
            flat[:m] = np.roll(INT_SPECIALS, seed + k)[:m]
            out.append(v.astype(np.int32))
        else:
            v = (rng.standard_normal((B, Hin, Win)) * 100).astype(f32)
            flat = v.reshape(-1)
            if k == 0:      # one NaN source per pixel
                flat[(seed * 7) % flat.size] = np.nan
                if flat.size > 1:
                    flat[(seed * 7 + 1) % flat.size] = -0.0
            elif flat.size > 2:
                flat[(seed * 7 + 2) % flat.size] = np.inf if k == 1 else -0.0
            out.append(v)
    return out


def words(v, big_endian):
    """the 32-bit words as they lie in device memory, in an int32 array (FITS byte order when big_endian)"""
    w = np.ascontiguousarray(v).view(np.uint32)
    return (w.byteswap() if big_endian else w).view(np.int32)


def place(v, res):
    """reshape_img_to_res: centred zero pad / crop with floor(diff / 2) on each axis"""
    B, Hs, Ws = v.shape
    out = np.zeros((B, res, res), f32)
    sl = []
    for n in (Hs, Ws):
        lo = int(np.floor((res - n) / 2.0))
        sl.append((slice(lo, lo + n), slice(0, n)) if lo >= 0 else (slice(0, res), slice(-lo, -lo + res)))
    out[:, sl[0][0], sl[1][0]] = v[:, sl[0][1], sl[1][1]]
    inside = np.zeros((res, res), bool)
    inside[sl[0][0], sl[1][0]] = True
    return out, inside


def ref_compose(planes, mask, s, res):
    """(img + agn) + bkg in fp32, * mask, nearest x s with / s^2, pad or crop"""
    with np.errstate(all="ignore"):
        v = planes[0].astype(f32)
        for p in planes[1:]:
            v = v + p.astype(f32)
        if mask is not None:
            v = v * mask.astype(f32)[None]
        if s > 1:
            v = np.repeat(np.repeat(v, s, axis=1), s, axis=2) / f32(s * s)
    return place(v, res)


def run_compose_input(planes_w, is_int32, be, mask_t, B, Hin, Win, s, res, norm=None):
    """xsd_compose_input from guarded, read-only word buffers into a NaN-filled guarded output; returns (rc, out [B][res][res])"""
    L = _lib()
    items = {k: w.view(f32) for k, w in zip(("img", "agn", "bkg"), planes_w)}
    g = Guarded(ro=tuple(items), out=(B, res, res), **items)
    mv, mode = norm if norm else (0.0, "linear")
    rc = L.xsd_compose_input(g.ptr("img"), g.ptr("agn"), g.ptr("bkg"), int(is_int32), int(be), mask_t.data_ptr() if mask_t is not None else None,
                             g.ptr("out"), B, Hin, Win, s, res, int(norm is not None), mv, STRETCH[mode] if isinstance(mode, str) else mode, _stream())
    torch.cuda.synchronize()
    g.check()
    return rc, g.np("out")


def run_compose_batch(pool_w, idx, is_int32, be, mask_t, Hin, Win, s, res, norm=None, n_slots=None, slot_elems=None):
    """xsd_compose_batch from a guarded, read-only pool [n_slots][slot_elems]; idx = (img, agn or None, bkg or None) host int32 arrays"""
    L = _lib()
    g = Guarded(ro=("pool",), pool=pool_w.view(f32), out=(len(idx[0]), res, res))
    mv, mode = norm if norm else (0.0, "linear")
    arr = [None if a is None else np.ascontiguousarray(a, np.int32) for a in idx]
    rc = L.xsd_compose_batch(g.ptr("pool"), int(is_int32), int(be), pool_w.shape[1] if slot_elems is None else slot_elems,
                             pool_w.shape[0] if n_slots is None else n_slots, *[None if a is None else a.ctypes.data for a in arr],
                             mask_t.data_ptr() if mask_t is not None else None, g.ptr("out"), len(arr[0]), Hin, Win, s, res, int(norm is not None), mv,
                             STRETCH[mode] if isinstance(mode, str) else mode, _stream())
    torch.cuda.synchronize()
    g.check()
    return rc, g.np("out")


# ---- geometry: bit for bit against fp32 numpy -------------------------------------------------------------------------------------------
GEOMETRIES = [(1, 1, 1, 1), (1, 1, 1, 4), (5, 7, 1, 8), (5, 7, 1, 4), (20, 13, 1, 16), (7, 5, 2, 9), (7, 5, 3, 16), (6, 6, 2, 12), (3, 4, 3, 5),
              (9, 11, 1, 513)]      # the last: 263,169 pixels > 1024 x 256, the second stride of compose_batch's x-grid


@pytest.mark.parametrize("Hin,Win,s,res", GEOMETRIES)
def test_compose_geometry_bit_for_bit(Hin, Win, s, res):
    rng = np.random.default_rng(Hin * 1000 + Win * 100 + s * 10 + res)
    mask = rng.integers(0, 2, size=(Hin, Win)).astype(np.uint8)
    mask_t = torch.from_numpy(mask).cuda()
    seed = 0
    for is_int32 in (True, False):
        for be in (False, True):
            for use_mask in (False, True):
                for extra in (0, 1, 2):
                    for B in (1, 2):
                        seed += 1
                        planes = make_planes(rng, 1 + extra, B, Hin, Win, is_int32, seed)
                        what = f"{'int32' if is_int32 else 'float32'} {'big-endian' if be else 'native'} mask {use_mask} extra {extra} B {B}"
                        want, inside = ref_compose(planes, mask if use_mask else None, s, res)
                        pw = [words(p, be) for p in planes]
                        rc, got = run_compose_input(pw, is_int32, be, mask_t if use_mask else None, B, Hin, Win, s, res)
                        assert rc == 0
                        same(got, want, "compose_input " + what)
                        assert not got[:, ~inside].view(np.uint32).any(), "outside the source rectangle: +0.0"
                        # the same slots through the batched gather: sample b takes slots b, B + b, 2 B + b
                        pool = np.stack([p.reshape(B, -1) for p in pw]).reshape((1 + extra) * B, Hin * Win)
                        idx = [np.arange(B) + k * B if k <= extra else None for k in range(3)]
                        rc, got_b = run_compose_batch(pool, idx, is_int32, be, mask_t if use_mask else None, Hin, Win, s, res)
                        assert rc == 0
                        same(got_b, got, "compose_batch against compose_input, " + what)
    assert torch.equal(mask_t.cpu(), torch.from_numpy(mask))


def test_compose_input_second_pass_of_the_grid():
    """B = 3, res = 419: 526,683 outputs > 2048 x 256 threads"""
    rng = np.random.default_rng(5)
    B, Hin, Win, s, res = 3, 150, 141, 3, 419
    mask = rng.integers(0, 2, size=(Hin, Win)).astype(np.uint8)
    planes = make_planes(rng, 3, B, Hin, Win, True, 1)
    want, _ = ref_compose(planes, mask, s, res)
    rc, got = run_compose_input([words(p, True) for p in planes], True, True, torch.from_numpy(mask).cuda(), B, Hin, Win, s, res)
    assert rc == 0 and B * res * res > 2048 * 256
    same(got, want, "compose_input, 419 x 419 x 3")


def test_compose_batch_chunk_boundary_absent_planes_and_slack():
    """B = 129 splits at COMPOSE_BATCH_CHUNK = 128; agn = -1 for some samples, bkg for others; slots longer than Hin x Win with NaN words
    in the slack, which nothing may read"""
    rng = np.random.default_rng(6)
    B, Hin, Win, s, res, n_slots, slot = 129, 5, 7, 1, 8, 40, 5 * 7 + 13
    vals = (rng.standard_normal((n_slots, Hin, Win)) * 50).astype(f32)
    pool_v = np.full((n_slots, slot), np.nan, f32)
    pool_v[:, :Hin * Win] = vals.reshape(n_slots, -1)
    mask = rng.integers(0, 2, size=(Hin, Win)).astype(np.uint8)
    mask_t = torch.from_numpy(mask).cuda()
    img = rng.integers(0, n_slots, B)
    agn = np.where(np.arange(B) % 3 == 0, -1, rng.integers(0, n_slots, B))
    bkg = np.where(np.arange(B) % 5 == 1, -1, rng.integers(0, n_slots, B))
    agn[128], bkg[128] = 7, -1       # the sample behind the chunk boundary has its own combination
    for be in (False, True):
        rc, got = run_compose_batch(words(pool_v, be), (img, agn, bkg), False, be, mask_t, Hin, Win, s, res)
        assert rc == 0 and not np.isnan(got).any()
        for b in range(B):
            planes = [vals[i][None] for i in (img[b], agn[b], bkg[b]) if i >= 0]
            want, _ = ref_compose(planes, mask, s, res)
            same(got[b:b + 1], want, f"sample {b} (slots {img[b]}, {agn[b]}, {bkg[b]})")
        # and against compose_input on the slots stacked by hand, group by group of equal presence
        for has_a in (False, True):
            for has_b in (False, True):
                grp = np.nonzero(((agn >= 0) == has_a) & ((bkg >= 0) == has_b))[0]
                stacks = [words(vals[img[grp]], be)] + ([words(vals[agn[grp]], be)] if has_a else [None]) + ([words(vals[bkg[grp]], be)] if has_b else [None])
                L = _lib()
                items = {k: w.view(f32) for k, w in zip(("img", "agn", "bkg"), stacks) if w is not None}
                g = Guarded(ro=tuple(items), out=(len(grp), res, res), **items)
                assert L.xsd_compose_input(g.ptr("img"), g.ptr("agn"), g.ptr("bkg"), 0, int(be), mask_t.data_ptr(), g.ptr("out"), len(grp), Hin, Win, s, res,
                                           0, 0.0, 0, _stream()) == 0
                torch.cuda.synchronize()
                g.check()
                same(got[grp], g.np("out"), f"compose_batch against compose_input, agn {has_a} bkg {has_b}")


def test_wrappers_agree_with_the_raw_entries():
    """engine.compose_input / compose_batch / image_upsample / normalize are what the package calls: the same bits as the raw library"""
    from xmm_superres_denoise import engine
    rng = np.random.default_rng(8)
    B, Hin, Win, s, res = 2, 7, 5, 2, 9
    planes = make_planes(rng, 3, B, Hin, Win, True, 3)
    mask = rng.integers(0, 2, size=(Hin, Win)).astype(np.uint8)
    mask_t = torch.from_numpy(mask).cuda()
    want, _ = ref_compose(planes, mask, s, res)
    t = [torch.from_numpy(words(p, True)).cuda() for p in planes]
    same(engine.compose_input(t[0], t[1], t[2], mask_t, res, None, upsample=s, big_endian=True).cpu().numpy()[:, 0], want, "engine.compose_input")
    pool = torch.cat([x.reshape(B, -1) for x in t])
    got = engine.compose_batch(pool, np.arange(B), np.arange(B) + B, np.arange(B) + 2 * B, mask_t, Hin, Win, res, None, upsample=s)
    same(got.cpu().numpy()[:, 0], want, "engine.compose_batch")


# ---- ImageUpsample -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 4, 6), (1, 5, 7)])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_image_upsample_bit_for_bit(shape, s):
    from xmm_superres_denoise import engine
    rng = np.random.default_rng(s)
    x = (rng.standard_normal(shape) * 3).astype(f32)
    x.reshape(-1)[:3] = (np.nan, -0.0, np.inf)
    H, W = shape[-2:]
    with np.errstate(all="ignore"):
        want = (torch.from_numpy(x).repeat_interleave(s, -2).repeat_interleave(s, -1) / f32(s * s)).numpy()
    g = Guarded(ro=("x",), x=x, out=tuple(shape[:-2]) + (H * s, W * s))
    assert _lib().xsd_image_upsample(g.ptr("x"), g.ptr("out"), x.size // (H * W), H, W, s, _stream()) == 0
    torch.cuda.synchronize()
    g.check()
    same(g.np("out"), want, "xsd_image_upsample")
    same(engine.image_upsample(torch.from_numpy(x).cuda(), s).cpu().numpy(), want, "engine.image_upsample")


# ---- Normalize -----------------------------------------------------------------------------------------------------------------------------
MAX_VALS = (0.0022336, 0.0005584, 1.0)


def clamp(v, lo, hi):
    """torch.clamp's selects in numpy: a NaN and a -0.0 at the lower bound pass through"""
    v = np.asarray(v)
    return np.where(v < lo, v.dtype.type(lo), np.where(v > hi, v.dtype.type(hi), v))


def forward_inputs(mv):
    m = f32(mv)
    ramp = (np.linspace(-0.1, 1.4, 6001) * mv).astype(f32)
    sp = np.array([0.0, -0.0, 1e-45, m, np.nextafter(m, f32(np.inf)), np.nextafter(m, f32(-np.inf)), np.inf, -np.inf, np.nan], f32)
    return np.concatenate([sp, ramp, sp])


def inverse_inputs():
    ramp = np.linspace(-0.1, 1.2, 6001).astype(f32)
    sp = np.array([0.0, 1.0, np.nextafter(f32(1), f32(0)), -1.1754944e-38, 1.0 + 2.0 ** -23, np.nan], f32)
    return np.concatenate([sp, ramp, sp])


def ref_stretch(v, mode, inverse, xp):
    """the reference's formulas on numpy float64 (xp = np) or on fp32 torch CPU tensors (xp = torch), as transforms/normalize.py writes them"""
    if xp is np:
        a_s, a_l, t = 0.02, 1000.0, (lambda z: z)
    else:
        a_s, a_l, t = torch.tensor(0.02), torch.tensor(1000), (lambda z: torch.as_tensor(z))
    if not inverse:
        return {"linear": lambda: v, "sqrt": lambda: xp.sqrt(v), "asinh": lambda: xp.asinh(v / a_s) / xp.asinh(t(1.0) / a_s),
                "log": lambda: xp.log(a_l * v + 1) / xp.log(t(a_l))}[mode]()
    return {"linear": lambda: v, "sqrt": lambda: v * v, "asinh": lambda: a_s * xp.sinh(v * xp.asinh(t(1.0) / a_s)),
            "log": lambda: ((a_l ** v if xp is np else torch.pow(a_l, v)) - 1) / a_l}[mode]()


def ref_normalize64(x, mv, mode, inverse):
    """float64 throughout, from the fp32 input and the fp32 max_val"""
    with np.errstate(all="ignore"):
        v, m = x.astype(np.float64), float(f32(mv))
        if not inverse:
            return clamp(ref_stretch(clamp(v, 0.0, m) / m, mode, False, np), 0.0, 1.0)
        return clamp(m * ref_stretch(v, mode, True, np), 0.0, m)


def ref_normalize_torch32(x, mv, mode, inverse):
    """the reference's own code path in fp32 on the CPU (Normalize.normalize_image with max_val > 0 / denormalize_image)"""
    img, m = torch.from_numpy(x.copy()), torch.tensor(mv)
    if not inverse:
        torch.clamp_(img, min=torch.tensor(0.0), max=m)
        img = ref_stretch(img / m, mode, False, torch)
        torch.clamp_(img, min=0.0, max=1.0)
        return img.numpy()
    img = m * ref_stretch(img, mode, True, torch)
    torch.clamp_min_(img, min=torch.tensor(0.0))
    torch.clamp_max_(img, max=m)
    return img.numpy()


def run_normalize(x, mv, mode, inverse):
    g = Guarded(ro=("x",), x=x, out=x.shape)
    rc = _lib().xsd_normalize(g.ptr("x"), g.ptr("out"), x.size, mv, STRETCH[mode] if isinstance(mode, str) else mode, int(inverse), _stream())
    torch.cuda.synchronize()
    g.check()
    return rc, g.np("out")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("mode", ["linear", "sqrt", "asinh", "log"])
@pytest.mark.parametrize("mv", MAX_VALS)
def test_normalize_stand_alone(mv, mode, inverse):
    x = inverse_inputs() if inverse else forward_inputs(mv)
    rc, got = run_normalize(x, mv, mode, inverse)
    assert rc == 0
    m = f32(mv)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan), "NaN exactly where the input is NaN"
    ok = got[~nan]
    assert (ok >= 0).all() and (ok <= (m if inverse else 1)).all()
    y32 = ref_normalize_torch32(x, mv, mode, inverse)
    with np.errstate(all="ignore"):
        if mode == "linear":      # clamp, one division, clamp (inverse: one product, clamp), every step fp32
            want = clamp(m * x, f32(0), m) if inverse else clamp(clamp(x, f32(0), m) / m, f32(0), f32(1))
            same(want, y32, "numpy restatement against the reference's torch code")       # -0.0 included: clamp_ keeps it
            same(got, want, f"linear, max_val {mv}, inverse {inverse}")
            return
        if mode == "sqrt":        # at most 1 ulp from the float64 result rounded to fp32
            c = (x * x) if inverse else clamp(x, f32(0), m) / m
            r = clamp(m * c, f32(0), m) if inverse else clamp(np.sqrt(c.astype(np.float64)).astype(f32), f32(0), f32(1))
            zero = (r == 0) & ~nan       # a zero keeps its sign (sqrt(-0.0) = -0.0, and clamp_ keeps it); the ulp distance is taken elsewhere
            assert np.array_equal(got[zero].view(np.uint32), r[zero].view(np.uint32)), "sign of zero"
            nan = nan | zero
            d = np.abs(got[~nan].view(np.int32).astype(np.int64) - r[~nan].view(np.int32).astype(np.int64))
            print(f"sqrt max_val {mv} inverse {inverse}: {100.0 * (d == 0).mean():.2f} % exact, max {d.max()} ulp")
            assert d.max() <= 1
            return
    y64 = ref_normalize64(x, mv, mode, inverse)
    rms32 = _assert_within_2x_of_fp32(got[~nan], y32[~nan], y64[~nan], f"{mode} max_val {mv} inverse {inverse}")
    assert rms32 > 0
    e, e32 = np.abs(got[~nan] - y64[~nan]), np.abs(y32[~nan] - y64[~nan])
    print(f"ratio to the reference's fp32 torch evaluation: {mode} max_val {mv} {'inverse' if inverse else 'forward'}: "
          f"rms {float(np.sqrt((e ** 2).mean())) / rms32:.3f} max {float(e.max() / e32.max()):.3f}")


@pytest.mark.parametrize("mode", ["linear", "sqrt", "asinh", "log"])
def test_fused_normalize_equals_stand_alone_on_the_unfused_output(mode):
    """compose_input / compose_batch with do_normalize against xsd_normalize applied to their own un-normalised output, bit for bit:
    padded zeros, a crop through an upsampled pixel, NaN, inf and -0.0 words included"""
    for mv in MAX_VALS:
        x = forward_inputs(mv)
        x = x[:6018]
        for (B, Hin, Win, s, res) in ((1, 59, 102, 1, 110), (2, 51, 59, 3, 150)):
            planes = [x[:B * Hin * Win].reshape(B, Hin, Win) * f32(s * s)]
            pw = [words(planes[0], True)]
            rc, plain = run_compose_input(pw, False, True, None, B, Hin, Win, s, res)
            assert rc == 0
            rc, want = run_normalize(plain, mv, mode, False)
            assert rc == 0
            rc, fused = run_compose_input(pw, False, True, None, B, Hin, Win, s, res, norm=(mv, mode))
            assert rc == 0
            same(fused, want, f"compose_input fused {mode} max_val {mv} upsample {s}")
            rc, fused_b = run_compose_batch(pw[0].reshape(B, -1), (np.arange(B), None, None), False, True, None, Hin, Win, s, res, norm=(mv, mode))
            assert rc == 0
            same(fused_b, want, f"compose_batch fused {mode} max_val {mv} upsample {s}")
            ok = fused[~np.isnan(fused)]
            assert (ok >= 0).all() and (ok <= 1).all() and np.isnan(fused).sum() == np.isnan(plain).sum()


# ---- refusals: each leaves the output's NaN fill untouched ------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    L = _lib()
    Hin, Win, res, n_slots = 5, 7, 8, 4
    pool = np.arange(n_slots * Hin * Win, dtype=np.int32).reshape(n_slots, Hin * Win)
    one = [pool[:1].reshape(1, Hin, Win)]
    ok_idx = (np.array([0, 1]), np.array([2, -1]), None)
    # max_val <= 0 (or NaN) on the fused path
    for mv in (0.0, -1.0, float("nan")):
        rc, out = run_compose_input(one, True, False, None, 1, Hin, Win, 1, res, norm=(mv, "linear"))
        assert rc == ERR_ARG and np.isnan(out).all()
        rc, out = run_compose_batch(pool, ok_idx, True, False, None, Hin, Win, 1, res, norm=(mv, "sqrt"))
        assert rc == ERR_ARG and np.isnan(out).all()
        rc, out = run_normalize(np.ones(16, f32), mv, "linear", False)
        assert rc == ERR_ARG and np.isnan(out).all()
        g = Guarded(ro=("x",), x=pool[:1].view(f32), out=(1, res, res))
        assert L.xsd_mask_pad_normalize(g.ptr("x"), 1, None, g.ptr("out"), 1, Hin, Win, res, 1, mv, 0, _stream()) == ERR_ARG
        torch.cuda.synchronize()
        g.check()
        assert np.isnan(g.np("out")).all()
    # a stretch outside 0..3
    for mode in (-1, 4):
        rc, out = run_compose_input(one, True, False, None, 1, Hin, Win, 1, res, norm=(1.0, mode))
        assert rc == ERR_ARG and np.isnan(out).all()
        rc, out = run_compose_batch(pool, ok_idx, True, False, None, Hin, Win, 1, res, norm=(1.0, mode))
        assert rc == ERR_ARG and np.isnan(out).all()
        rc, out = run_normalize(np.ones(16, f32), 1.0, mode, False)
        assert rc == ERR_ARG and np.isnan(out).all()
    # slots shorter than the image
    rc, out = run_compose_batch(pool, ok_idx, True, False, None, Hin, Win, 1, res, slot_elems=Hin * Win - 1)
    assert rc == ERR_ARG and np.isnan(out).all()
    # an index outside the pool: the message names the sample
    for idx in ((np.array([0, n_slots]), None, None), (np.array([0, -1]), None, None), (np.array([0, 1]), np.array([0, -2]), None),
                (np.array([0, 1]), None, np.array([n_slots, 0]))):
        rc, out = run_compose_batch(pool, idx, True, False, None, Hin, Win, 1, res)
        assert rc == ERR_ARG and np.isnan(out).all()
        assert b"sample" in L.xsd_last_error()
    # upsample < 1
    for s in (0, -2):
        rc, out = run_compose_input(one, True, False, None, 1, Hin, Win, s, res)
        assert rc == ERR_ARG and np.isnan(out).all()
        rc, out = run_compose_batch(pool, ok_idx, True, False, None, Hin, Win, s, res)
        assert rc == ERR_ARG and np.isnan(out).all()
        g = Guarded(ro=("x",), x=np.ones((1, 4, 6), f32), out=(1, 8, 12))
        assert L.xsd_image_upsample(g.ptr("x"), g.ptr("out"), 1, 4, 6, s, _stream()) == ERR_ARG
        torch.cuda.synchronize()
        g.check()
        assert np.isnan(g.np("out")).all()
    # and the accepted call next to them still works
    rc, out = run_compose_batch(pool, ok_idx, True, False, None, Hin, Win, 1, res)
    assert rc == 0 and not np.isnan(out).any()
