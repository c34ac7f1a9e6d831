"""The 7 kernels of csrc/fsim.hip and the host-built plan, one by one, through xsd_fsim_test_stage: after an eval the hook copies one
region of the workspace (pooled, eo, en, an, a0sq, T, the tile partials of fsim_map) or of the plan (the 16 log-Gabor filters, the noise
constants) out.  cgemm and the median have tests of their own in test_hip_fsim.py (test_dft2_alone, test_median_alone); here cgemm is
also covered in place, with the filters multiplied in, through `eo`.

The yardstick is tests/golden/fsim_torch.py returning MAPS (pc_maps, fsim_maps: the same code as the restatement, which
`test_reference_maps_reduce_to_the_restatement` asserts), in float64; f32 = the same in float32 on the same fp32-representable inputs.
  plan (filters, noise constants), per element   max(2 |f32 - f64|, 1e-12): the engine builds them in double on the host, and so does the
        yardstick, so they differ by libm alone: a few ulp in the argument of exp(-(log r / w0)^2 / ...), which reaches ~700 before the
        value underflows, i.e. < 700 * 4 * 2.2e-16 = 6e-13 of values that are at most 1.  The measured distance is in DESIGN.md section 24.
  pooled                                         2 double ulp at the map's scale (max |f64|)
  eo, en, an, a0sq, per pixel                    2 * max over the map |f32 - f64|
  T, per (image, orientation)                    max(2 |f32 - f64|, 5e-6 max(1, |f64|)); and T from the engine's OWN a0sq by torch.median and
                                                 the written formula with the engine's own noise constants, 1e-12 relative
  fsim_map tile partials                         max(2 max over the tiles |f32_tile - f64_tile|, 5e-6 max(1, |f64_tile|))
  fsim_finish                                    sum of the engine's own partials, num / den, 1e-12 relative
Before every eval the workspace is poisoned by an eval of all-NaN images of the same shape, and the hook's destination is NaN-filled."""
import ctypes

import pytest
import torch

import ext_metrics_torch as E
import fsim_torch as Fs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 61x53 odd / odd, 64x48 even / even, two tile columns in either notation (w = 130), and the longest row the engine takes (1024: 16 tile
# columns, 164 pc_point blocks; a pooled side of 1030 is refused, see test_stage_refusals)
SHAPES = [(61, 53), (64, 48), (130, 41), (41, 130), (41, 1024)]
PLAN_SHAPES = [(53, 61), (48, 64), (3, 3), (7, 4)]
POOL_SHAPES = [(61, 53), (384, 385), (641, 650), (640, 643)]          # ks = 1, 2 (tie 1.5), 3, 2 (tie 2.5: Python's round goes to even)
B = 2
WORST = {}
_ref, _eng = {}, {}


def _id(shape):
    return f"{shape[0]}x{shape[1]}"


def _note(stage, err, bar, shape):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    if stage not in WORST or ratio > WORST[stage][0]:
        WORST[stage] = (ratio, _id(shape))
    return ratio


def pair(shape, n=B):
    p, t = Fs.photon_pair((n,) + tuple(shape), torch.Generator().manual_seed(100 + shape[0] + shape[1]))
    return p.float(), t.float()


def reference(shape):
    if shape not in _ref:
        p, t = pair(shape)
        _ref[shape] = {"p": p, "t": t, "r64": Fs.fsim_maps(p.double(), t.double()), "r32": Fs.fsim_maps(p, t)}
    return _ref[shape]


@pytest.fixture(scope="module")
def engine():
    from xmm_superres_denoise.engine import FsimEngine
    with torch.cuda.device(DEV):
        return FsimEngine()


def run(engine, p, t, regions):
    nan = torch.full_like(p, float("nan")).to(DEV)
    engine.eval(nan, nan)
    out = engine.eval(p.to(DEV), t.to(DEV))
    st = {}
    for name in regions:
        dtype = torch.float32 if name in ("eo", "a0sq") else torch.float64
        n = {"eo": 64, "en": 8, "an": 8, "a0sq": 8, "filt": 16}.get(name, 2) * p.numel() + 64
        buf = torch.full((n,), float("nan"), device=DEV, dtype=dtype)
        got, info = engine.stage(name, out=buf)
        assert torch.isnan(buf[got.numel():]).all()                   # nothing past the region
        st[name] = (got.cpu(), info)
    return {"out": out.cpu(), "stage": st}


def results(engine, shape):
    if shape not in _eng:
        c = reference(shape)
        _eng[shape] = run(engine, c["p"], c["t"], ("pooled", "eo", "en", "an", "a0sq", "T", "part", "filt", "noise"))
    return _eng[shape]


def _both(c, which, key):
    """[2B, ...]: the reference's map of preds then target, as the engine orders sb = s * B + image"""
    return torch.cat([c[which]["pc"][0][key], c[which]["pc"][1][key]])


def test_reference_maps_reduce_to_the_restatement():
    for shape in ((61, 53), (64, 48)):
        c = reference(shape)
        p, t = c["p"].double(), c["t"].double()
        n, d = Fs.fsim_parts(p, t)
        assert bool(((c["r64"]["num"].sum(dim=[1, 2]) - n).abs() <= 1e-12 * n.abs()).all()) and bool(((c["r64"]["den"].sum(dim=[1, 2]) - d).abs() <= 1e-12 * d).all())
        pc, parts = Fs.phase_congruency(Fs.pool(p[:, None]), parts=True)
        m = c["r64"]["pc"][0]
        assert bool(((m["pc"] - pc[:, 0]).abs() <= 1e-12 * pc[:, 0].abs()).all()) and bool(((m["T"] - parts["T"]).abs() <= 1e-12 * parts["T"]).all())
        assert torch.equal(m["eo"], parts["eo"])


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=_id)
def test_plan_filters_and_noise_constants(engine, shape):
    h, w = shape
    x = torch.rand((1, h, w), generator=torch.Generator().manual_seed(h * w))
    e = run(engine, x, x.flip(1).contiguous(), ("filt", "noise"))
    filt, info = e["stage"]["filt"]
    assert (info["B"], info["h"], info["w"]) == (16, h, w) and tuple(filt.shape) == (16, h, w)
    f64 = Fs.construct_filters(h, w, torch.float64)
    f32 = Fs.construct_filters(h, w, torch.float32)
    err = (filt.reshape(4, 4, h, w) - f64).abs()
    bar = torch.clamp(2 * (f32.double() - f64).abs(), min=1e-12)
    print(f"plan {h}x{w} filters: max |engine - f64| {float(err.max()):.3e} (max |f32 - f64| {float((f32.double() - f64).abs().max()):.3e}) "
          f"worst err/bar {_note('filt', float(err.max()), 1e-12, shape):.4f} vs the 1e-12 floor")
    assert bool((err <= bar).all()), float(err.max())
    assert float(filt[:, 0, 0].abs().max()) == 0.0                    # no DC
    noise, _ = e["stage"]["noise"]
    n64 = torch.stack(Fs.noise_constants(f64))
    n32 = torch.stack(Fs.noise_constants(f32)).double()
    assert tuple(noise.shape) == (3, 4)
    nerr, nbar = (noise - n64).abs(), torch.clamp(2 * (n32 - n64).abs(), min=1e-12 * n64.abs())
    print(f"plan {h}x{w} noise constants: max rel |engine - f64| {float((nerr / n64.abs()).max()):.3e} (f32 restatement {float(((n32 - n64).abs() / n64.abs()).max()):.3e})")
    _note("noise", float((nerr / n64.abs()).max()), 1e-12, shape)
    assert bool((nerr <= nbar).all()), (noise, n64)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_id)
def test_pool_kernel(engine, shape):
    H, W = shape
    ks = Fs.kernel_size(H, W)
    assert ks == {61: 1, 384: 2, 641: 3, 640: 2}[H] and (H % ks or W % ks or ks == 1)           # a remainder is dropped
    p, t = pair(shape, 1)
    e = run(engine, p, t, ("pooled",))
    got, info = e["stage"]["pooled"]
    want = torch.cat([Fs.pool(p.double()[:, None])[:, 0], Fs.pool(t.double()[:, None])[:, 0]])
    assert tuple(got.shape) == tuple(want.shape) == (2, H // ks, W // ks) and (info["h"], info["w"]) == (H // ks, W // ks)
    assert torch.isfinite(got).all(), "an element was not written"
    scale = float(want.abs().max())
    ulp = float(torch.nextafter(torch.tensor(scale, dtype=torch.float64), torch.tensor(float("inf"), dtype=torch.float64))) - scale
    err = float((got - want).abs().max())
    print(f"pool {H}x{W} ks {ks}: max |engine - f64| {err:.3e}, 2 ulp at {scale:.1f} = {2 * ulp:.3e} ratio {_note('pooled', err, 2 * ulp, shape):.3f}")
    assert err <= 2 * ulp


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_responses_per_pixel(engine, shape):
    c, e = reference(shape), results(engine, shape)
    h, w = shape
    misses = []
    for name in ("eo", "en", "an", "a0sq"):
        got, info = e["stage"][name]
        f64, f32 = _both(c, "r64", name), _both(c, "r32", name)
        if name == "eo":
            got = torch.view_as_complex(got.double().reshape(2 * B, 4, 4, h, w, 2).contiguous())
            f32 = f32.to(torch.complex128)
        else:
            got, f32 = got.double(), f32.double()
        assert tuple(got.shape) == tuple(f64.shape) and info["B"] == 2 * B and (info["h"], info["w"]) == (h, w)
        assert torch.isfinite(torch.view_as_real(got) if name == "eo" else got).all(), (name, "an element was not written")
        bar = 2 * float((f32 - f64).abs().max())
        err = float((got - f64).abs().max())
        print(f"{_id(shape)} {name}: max |engine - f64| {err:.3e} bar 2 max|f32 - f64| {bar:.3e} (max |f64| {float(f64.abs().max()):.3e}) ratio {_note(name, err, bar, shape):.3f}")
        if not err <= bar:
            misses.append((name, err, bar))
    assert not misses, misses


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_threshold_T(engine, shape):
    c, e = reference(shape), results(engine, shape)
    T, _ = e["stage"]["T"]
    t64, t32 = _both(c, "r64", "T"), _both(c, "r32", "T").double()
    assert tuple(T.shape) == (2 * B, 4) and torch.isfinite(T).all()
    bar = torch.clamp(2 * (t32 - t64).abs(), min=0).maximum(5e-6 * t64.abs().clamp_min(1.0))
    err = (T - t64).abs()
    print(f"{_id(shape)} T: max |engine - f64| {float(err.max()):.3e} worst err/bar {_note('T', float((err / bar).max()), 1.0, shape):.3f}")
    assert bool((err <= bar).all()), (T, t64)
    # median_T_kernel alone: the engine's own fp32 a0sq through torch.median and the written formula with the engine's own constants
    a0sq, noise = e["stage"]["a0sq"][0], e["stage"]["noise"][0]
    med = torch.median(a0sq.reshape(2 * B, 4, -1), dim=-1).values.double()
    own = Fs.threshold(med, noise[0][None], noise[1][None], noise[2][None])
    rel = float(((T - own).abs() / own.abs()).max())
    print(f"{_id(shape)} T from the engine's own a0sq: max rel {rel:.3e}")
    _note("T(own a0sq)", rel, 1e-12, shape)
    assert rel <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_fsim_map_tile_partials_and_finish(engine, shape):
    c, e = reference(shape), results(engine, shape)
    h, w = shape
    part, info = e["stage"]["part"]
    assert (info["tile_h"], info["tile_w"], info["entries"]) == (4, 64, 2) and info["tiles_x"] == -(-w // 64) and info["ntiles"] == info["tiles_x"] * -(-h // 4)
    assert tuple(part.shape) == (B, info["ntiles"], 2) and torch.isfinite(part).all()
    misses = []
    for k, name in enumerate(("num", "den")):
        t64, t32 = E.tile_sums(c["r64"][name], 4, 64), E.tile_sums(c["r32"][name].double(), 4, 64)
        yard = 2 * float((t32 - t64).abs().max())
        bar = torch.clamp(5e-6 * t64.abs().clamp_min(1.0), min=yard)
        err = (part[:, :, k] - t64).abs()
        print(f"{_id(shape)} fsim_map {name}: worst |engine - f64| {float(err.max()):.3e} (2|f32-f64| {yard:.3e}) worst err/bar "
              f"{_note('part[' + name + ']', float((err / bar).max()), 1.0, shape):.4f}")
        if not bool((err <= bar).all()):
            misses.append((name, float(err.max())))
    assert not misses, misses
    s = part.sum(1)
    want = s[:, 0] / s[:, 1]
    rel = float(((e["out"] - want).abs() / want.abs()).max())
    print(f"{_id(shape)} finish: {e['out'].tolist()} max rel {rel:.2e}")
    _note("finish", rel, 1e-12, shape)
    assert rel <= 1e-12
    # the second image alone is bitwise its batch-of-two self, stage by stage
    one = run(engine, c["p"][1:2], c["t"][1:2], ("pooled", "a0sq", "T", "part"))
    assert torch.equal(one["out"][0], e["out"][1]) and torch.equal(one["stage"]["part"][0][0], part[1])
    for name in ("pooled", "a0sq", "T"):
        assert torch.equal(one["stage"][name][0], e["stage"][name][0][[1, B + 1]]), name


def test_stage_refusals(engine):
    from xmm_superres_denoise.engine import FsimEngine, XsdError, _lib
    L = _lib.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    info = (ctypes.c_int32 * 8)()
    buf = torch.zeros(1 << 18, device=DEV)
    with torch.cuda.device(DEV):
        fresh = FsimEngine()
    assert L.xsd_fsim_test_stage(fresh.h, 0, buf.data_ptr(), buf.numel() * 4, info, stream) == -1
    assert b"has not evaluated" in L.xsd_last_error()
    with pytest.raises(XsdError, match="has not evaluated"):
        fresh.stage("pooled")
    with pytest.raises(XsdError, match="1024"):                        # a pooled side of 1030 is not taken
        fresh.eval(torch.zeros((1, 41, 1030), device=DEV), torch.zeros((1, 41, 1030), device=DEV))
    z = torch.rand((1, 9, 7), device=DEV)
    fresh.eval(z, z)
    ok = (fresh.h, 0, buf.data_ptr(), buf.numel() * 4, info, stream)
    assert L.xsd_fsim_test_stage(*ok) == 0 and list(info)[:4] == [2, 9, 7, 0]
    for i in (0, 2, 4):
        args = list(ok)
        args[i] = None
        assert L.xsd_fsim_test_stage(*args) == -1
        assert b"null pointer" in L.xsd_last_error()
    for stage in (-1, len(FsimEngine.STAGES)):
        assert L.xsd_fsim_test_stage(fresh.h, stage, buf.data_ptr(), buf.numel() * 4, info, stream) == -1
        assert b"unknown stage" in L.xsd_last_error()
    for name in FsimEngine.STAGES:
        s = FsimEngine.STAGES.index(name)
        full, _ = fresh.stage(name)
        need = full.numel() * full.element_size()
        buf.fill_(7.0)
        assert L.xsd_fsim_test_stage(fresh.h, s, buf.data_ptr(), need - 1, info, stream) == -1
        assert b"buffer too small" in L.xsd_last_error() and str(need).encode() in L.xsd_last_error()
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all())                               # a refused call copies nothing
        assert L.xsd_fsim_test_stage(fresh.h, s, buf.data_ptr(), need, info, stream) == 0
    with pytest.raises(XsdError, match="unknown stage"):
        fresh.stage("z")
    # the transform's scratch overwrites the regions: nothing to read back after test_dft2
    fresh.dft2(torch.zeros((1, 9, 7, 2), device=DEV))
    with pytest.raises(XsdError, match="has not evaluated"):
        fresh.stage("pooled")
    torch.cuda.synchronize()


def test_zz_worst_error_over_bar_per_stage():
    """not a check of its own: prints the table DESIGN.md section 24 quotes"""
    for stage in sorted(WORST):
        print(f"WORST {stage:16s} error/bar {WORST[stage][0]:.4f}  at {WORST[stage][1]}")
