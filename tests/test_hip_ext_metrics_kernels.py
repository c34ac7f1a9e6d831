"""The 8 kernels of csrc/ext_metrics.hip one by one (pool_chain, mdsi_pool, vif_decimate, gms, haarpsi, mdsi, vif_stats, finish),
through xsd_ext_metrics_test_stage: after an eval the hook copies one region of the workspace out -- an image of a chain or the per-tile
partial sums of a kernel -- and each is compared with the float64 MAPS of tests/golden/ext_metrics_torch.py (the same published
formulas as the restatement test_hip_ext_metrics.py uses; `test_reference_maps_reduce_to_the_restatement` ties the two).

Bars (f64 / f32 = the reference maps in the two dtypes on the same fp32-representable inputs; never taken from the engine):
  images, per pixel    |engine - f64| <= max(2 * max over the map |f32 - f64|, 1.2e-7 * max |f64|)
  tile partials        |engine - f64| <= max(2 * max over the map's tiles |f32_tile - f64_tile|, 5e-6 * max(1, |f64_tile|))
  accumulated values   |engine - f64| <= max(2 * |f32 - f64|, 5e-6 * max(1, |f64|))          (each one on its own, not in a ratio)
  finish               the six outputs = the written formulas applied in float64 to the engine's own partials, 1e-12 relative
Before every eval the workspace is poisoned by an eval of all-NaN images of the same shape, so an element a kernel does not write stays
NaN; the hook's destination is NaN-filled too."""
import ctypes

import pytest
import torch

import ext_metrics_torch as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGES = ("u1", "u2", "u3", "m", "v1", "v2", "v3")
PARTIALS = ("gms0", "gms1", "gms2", "gms3", "haar", "mdsi1", "mdsi2", "vif0", "vif1", "vif2", "vif3")
MDSI_REGIONS = ("m", "mdsi1", "mdsi2")
# the smallest shapes that reach each branch: one VIF window at scale 3; mixed parity at pool levels 0, 1, 2; the existing even and odd
# cases; two tile columns in gms scales 0, 1 and haarpsi; pool_chain with tiles_x = 2; 257 tiles (image_sum's strided loop)
SHAPES = [(41, 41), (41, 58), (58, 41), (44, 47), (64, 48), (61, 53), (41, 130), (41, 515), (1025, 41)]
MDSI_SHAPES = [(128, 128), (384, 384), (640, 640), (641, 641), (896, 896)]        # k = 1 (tie 0.5), 2 (tie 1.5), 2 (tie 2.5), 3 (odd), 4 (tie 3.5)
KIND_SHAPES = [(80, 80), (61, 53), (44, 47)]
KINDS = ("sources_on", "sources_off", "flat", "identical")
CASES = [("photon", s) for s in SHAPES] + [(k, s) for k in KINDS for s in KIND_SHAPES]
MDSI_CASES = [("photon", s) for s in MDSI_SHAPES]
B = 3
WORST = {}            # stage -> (error / bar, case): printed by the last test
_ref, _eng = {}, {}


def _id(case):
    return f"{case[0]}-{case[1][0]}x{case[1][1]}"


def make_pair(kind, shape, n=B):
    """fp32 (preds, target), [n, H, W]"""
    H, W = shape
    gen = torch.Generator().manual_seed(100 + H + W)
    if kind in ("photon", "identical"):
        p, t = E.photon_pair((n, H, W), gen)
        return (t.float(), t.float()) if kind == "identical" else (p.float(), t.float())
    t = torch.zeros((n, H, W), dtype=torch.float64)
    if kind == "flat":
        t += 0.25
    else:
        # zero background; 0.9 point sources every 16 pixels and two 3x3 sources; "on": at multiples of 16, which are the origins of the
        # 16 x 16-window VIF tiles and (rows: multiples of 4, columns 0 and 64) of the 64 x 4 pixel tiles; "off": moved by (8, 8) / (5, 7)
        o = 0 if kind == "sources_on" else 8
        t[:, o::16, o::16] = 0.9
        q = 0 if kind == "sources_on" else 5
        t[:, 16 + q:19 + q, 32 + q:35 + q] = 0.6
        if W > 67 + q + 2:
            t[:, 32 + q:35 + q, 64 + q + (0 if kind == "sources_on" else 2):67 + q + (0 if kind == "sources_on" else 2)] = 0.6
    p = torch.clamp(t + 0.05 * torch.randn((n, H, W), dtype=torch.float64, generator=gen), 0, 1)
    return p.float(), t.float()


def ref_maps(p, t, mdsi_only=False):
    """{region: map(s)} from the map-returning reference, in the dtype of p: images (preds, target); partial regions a list of maps, one
    per entry of the tile partial"""
    r = {}
    mx, my, re, im, dev = E.mdsi_maps(p, t)
    r["m"] = (mx, my)
    r["mdsi1"] = [re, im]
    r["mdsi2"] = [dev]
    if mdsi_only:
        return r
    up, ut = E.pool_levels(p), E.pool_levels(t)
    for k in range(3):
        r[f"u{k + 1}"] = (up[k], ut[k])
    ms, g1 = E.gms_maps(p, t)
    for k in range(4):
        z = torch.zeros_like(ms[k])
        r[f"gms{k}"] = [ms[k], ms[k] ** 2, g1 if k == 1 else z, g1 ** 2 if k == 1 else z]
    r["haar"] = list(E.haarpsi_maps(p, t))
    for k, (vp, vt, num, den) in enumerate(E.vif_maps(p, t)):
        if k:
            r[f"v{k}"] = (vp, vt)
        r[f"vif{k}"] = [num, den]
    return r


def _pstd(m):
    return ((m - m.mean(dim=[1, 2], keepdim=True)) ** 2).mean(dim=[1, 2]).sqrt()


def accumulated_from_maps(r, mdsi_only=False):
    """{name: [B] doubles}: every quantity the engine accumulates over an image, from the reference maps"""
    a = {"mdsi_re": r["mdsi1"][0].mean(dim=[1, 2]), "mdsi_im": r["mdsi1"][1].mean(dim=[1, 2]), "mdsi_dev": r["mdsi2"][0].mean(dim=[1, 2])}
    if not mdsi_only:
        for k in range(4):
            a[f"vif_num{k}"], a[f"vif_den{k}"] = r[f"vif{k}"][0].sum(dim=[1, 2]), r[f"vif{k}"][1].sum(dim=[1, 2])
            a[f"ms_gmsd_dev{k}"] = _pstd(r[f"gms{k}"][0])
        a["vif_num"], a["vif_den"] = sum(a[f"vif_num{k}"] for k in range(4)), sum(a[f"vif_den{k}"] for k in range(4))
        a["gmsd_dev"] = _pstd(r["gms1"][2])
        a["haar_num"], a["haar_den"] = r["haar"][0].sum(dim=[1, 2]), r["haar"][1].sum(dim=[1, 2])
    return {k: v.double() for k, v in a.items()}


def _pop_var(s, s2, n):
    v = s2 / n - (s / n) ** 2
    return torch.where(v < 0, torch.zeros_like(v), v)          # keeps a NaN


def accumulated_from_partials(e, mdsi_only=False):
    """the same quantities from the engine's own tile partials (float64 on the host)"""
    P = {k: e["stage"][k][0].sum(1) for k in (MDSI_REGIONS[1:] if mdsi_only else PARTIALS)}           # [B, entries]
    n = lambda k: float(e["stage"][k][1]["h"] * e["stage"][k][1]["w"])
    a = {"mdsi_re": P["mdsi1"][:, 0] / n("mdsi1"), "mdsi_im": P["mdsi1"][:, 1] / n("mdsi1"), "mdsi_dev": P["mdsi2"][:, 0] / n("mdsi2")}
    if not mdsi_only:
        for k in range(4):
            a[f"vif_num{k}"], a[f"vif_den{k}"] = P[f"vif{k}"][:, 0], P[f"vif{k}"][:, 1]
            a[f"ms_gmsd_dev{k}"] = _pop_var(P[f"gms{k}"][:, 0], P[f"gms{k}"][:, 1], n(f"gms{k}")).sqrt()
        a["vif_num"], a["vif_den"] = sum(a[f"vif_num{k}"] for k in range(4)), sum(a[f"vif_den{k}"] for k in range(4))
        a["gmsd_dev"] = _pop_var(P["gms1"][:, 2], P["gms1"][:, 3], n("gms1")).sqrt()
        a["haar_num"], a["haar_den"] = P["haar"][:, 0], P["haar"][:, 1]
    return a


def reference(case, mdsi_only=False):
    if case not in _ref:
        p, t = make_pair(*case)
        r64, r32 = ref_maps(p.double(), t.double(), mdsi_only), ref_maps(p, t, mdsi_only)
        _ref[case] = {"p": p, "t": t, "r64": r64, "r32": r32, "a64": accumulated_from_maps(r64, mdsi_only), "a32": accumulated_from_maps(r32, mdsi_only)}
    return _ref[case]


@pytest.fixture(scope="module")
def engine():
    from xmm_superres_denoise.engine import ExtMetricsEngine
    with torch.cuda.device(DEV):
        return ExtMetricsEngine()


def run(engine, p, t, regions=IMAGES + PARTIALS):
    """poison the workspace, eval, read every region back into NaN-filled buffers: {"out": [n, 6], "stage": {name: (tensor(s), info)}}"""
    nan = torch.full_like(p, float("nan")).to(DEV)
    engine.eval(nan, nan)
    out = engine.eval(p.to(DEV), t.to(DEV))
    st = {}
    for name in regions:
        if name in IMAGES:
            got = []
            for side in (0, 1):
                buf = torch.full((p.numel() + 64,), float("nan"), device=DEV)
                img, info = engine.stage(name, side, out=buf)
                got.append(img.cpu())
                assert torch.isnan(buf[img.numel():]).all()           # nothing past the region
            st[name] = (tuple(got), info)
        else:
            buf = torch.full((p.numel() + 64,), float("nan"), device=DEV, dtype=torch.float64)
            part, info = engine.stage(name, out=buf)
            assert torch.isnan(buf[part.numel():]).all()
            st[name] = (part.cpu(), info)
    return {"out": out.cpu(), "stage": st}


def engine_results(engine, case, mdsi_only=False):
    if case not in _eng:
        c = reference(case, mdsi_only)
        _eng[case] = run(engine, c["p"], c["t"], MDSI_REGIONS if mdsi_only else IMAGES + PARTIALS)
    return _eng[case]


def _note(stage, err, bar, case):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    if stage not in WORST or ratio > WORST[stage][0]:
        WORST[stage] = (ratio, _id(case))
    return ratio


def check_images(e, c, case, names):
    misses = []
    for name in names:
        (gx, gy), info = e["stage"][name]
        for side, g in enumerate((gx, gy)):
            f64, f32 = c["r64"][name][side], c["r32"][name][side].double()
            assert tuple(g.shape) == tuple(f64.shape) == (info["B"], info["h"], info["w"]), (name, g.shape, f64.shape, info)
            assert info["entries"] == 0 and torch.isfinite(g).all(), (name, "an element was not written")
            bar = max(2 * float((f32 - f64).abs().max()), 1.2e-7 * float(f64.abs().max()))
            err = float((g.double() - f64).abs().max())
            print(f"{_id(case)} image {name}[{side}] {tuple(g.shape)} max|engine-f64| {err:.3e} bar {bar:.3e} ratio {_note(name, err, bar, case):.2f}")
            if not err <= bar:
                misses.append((name, side, err, bar))
    assert not misses, misses


def check_partials(e, c, case, names):
    misses = []
    for name in names:
        part, info = e["stage"][name]
        th, tw = info["tile_h"], info["tile_w"]
        assert (th, tw) == ((16, 16) if name.startswith("vif") else (4, 64)) and info["entries"] == len(c["r64"][name])
        assert tuple(part.shape) == (info["B"], info["ntiles"], info["entries"])
        assert info["ntiles"] == info["tiles_x"] * -(-info["h"] // th) and info["tiles_x"] == -(-info["w"] // tw)
        assert torch.isfinite(part).all(), (name, "a tile slot was not written")
        for k, (m64, m32) in enumerate(zip(c["r64"][name], c["r32"][name])):
            assert tuple(m64.shape[1:]) == (info["h"], info["w"]), (name, m64.shape, info)
            t64, t32 = E.tile_sums(m64, th, tw), E.tile_sums(m32.double(), th, tw)
            yard = 2 * float((t32 - t64).abs().max())
            bar = torch.clamp(5e-6 * t64.abs().clamp_min(1.0), min=yard)
            err = (part[:, :, k] - t64).abs()
            worst = int((err / bar).argmax())
            ratio = _note(f"{name}[{k}]", float(err.reshape(-1)[worst]), float(bar.reshape(-1)[worst]), case)
            print(f"{_id(case)} partial {name}[{k}] tiles {tuple(t64.shape)} worst |engine-f64| {float(err.reshape(-1)[worst]):.3e} bar {float(bar.reshape(-1)[worst]):.3e} "
                  f"(2|f32-f64| {yard:.3e}) ratio {ratio:.3f}")
            if not bool((err <= bar).all()):
                misses.append((name, k, float(err.max()), float(bar.reshape(-1)[worst])))
    assert not misses, misses


def check_accumulated(e, c, case, mdsi_only=False):
    got = accumulated_from_partials(e, mdsi_only)
    misses = []
    for name, f64 in c["a64"].items():
        for b in range(f64.numel()):
            g, v64, v32 = float(got[name][b]), float(f64[b]), float(c["a32"][name][b])
            bar = max(2 * abs(v32 - v64), 5e-6 * max(1.0, abs(v64)))
            err = abs(g - v64)
            print(f"{_id(case)} image {b} {name:12s} f64 {v64:.10g} engine {g:.10g} |engine-f64| {err:.3e} |f32-f64| {abs(v32 - v64):.3e} bar {bar:.3e} "
                  f"ratio {_note(name, err, bar, case):.3f}")
            if not err <= bar:
                misses.append((name, b, g, v64, v32))
    assert not misses, misses


def finish_from_partials(e):
    """the six outputs by the written formulas, in float64, from the engine's own partials; also the radicands of the three roots"""
    a = accumulated_from_partials(e)
    w = torch.tensor(E.MS_GMSD_WEIGHTS, dtype=torch.float64)
    ms = sum(w[k] * a[f"ms_gmsd_dev{k}"] ** 2 for k in range(4))
    v = (a["haar_num"] + E.EPS32) / (a["haar_den"] + E.EPS32)
    want = torch.stack([a["gmsd_dev"], ms.sqrt(), (torch.log(v / (1 - v)) / 4.2) ** 2, a["mdsi_dev"] ** 0.25, a["vif_num"], a["vif_den"]], 1)
    return want, a


# ---- the reference itself
def test_reference_maps_reduce_to_the_restatement():
    for case in (("photon", (61, 53)), ("sources_on", (80, 80)), ("photon", (41, 58))):
        c = reference(case)
        p, t, a = c["p"].double(), c["t"].double(), c["a64"]
        want = {"vif_num": E.vif_parts(p, t)[0], "vif_den": E.vif_parts(p, t)[1], "haar_num": E.haarpsi_parts(p, t)[0], "haar_den": E.haarpsi_parts(p, t)[1],
                "gmsd_dev": E.gmsd(p, t), "mdsi_dev": E.mdsi_deviation(p, t)}
        for k in range(4):
            want[f"ms_gmsd_dev{k}"] = E.ms_gmsd_scales(p, t)[:, k]
        for name, v in want.items():
            assert bool(((a[name] - v).abs() <= 1e-12 * v.abs()).all()), (case, name, a[name], v)
        # and through the final formulas: the reference's accumulated values give all_metrics
        m = E.all_metrics(p, t)
        w = torch.tensor(E.MS_GMSD_WEIGHTS, dtype=torch.float64)
        v = (a["haar_num"] + E.EPS32) / (a["haar_den"] + E.EPS32)
        mine = {"gmsd": a["gmsd_dev"], "ms_gmsd": sum(w[k] * a[f"ms_gmsd_dev{k}"] ** 2 for k in range(4)).sqrt(), "haarpsi": (torch.log(v / (1 - v)) / 4.2) ** 2,
                "msdi": a["mdsi_dev"] ** 0.25, "vif_p": a["vif_num"] / a["vif_den"]}
        for name in E.NAMES:
            assert bool(((mine[name] - m[name]).abs() <= 1e-12 * m[name].abs()).all()), (case, name)


# ---- the stages
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_images(engine, case):
    check_images(engine_results(engine, case), reference(case), case, IMAGES)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tile_partials(engine, case):
    check_partials(engine_results(engine, case), reference(case), case, PARTIALS)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_accumulated_quantities(engine, case):
    check_accumulated(engine_results(engine, case), reference(case), case)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_finish(engine, case):
    e = engine_results(engine, case)
    want, a = finish_from_partials(e)
    got = e["out"]
    if case[0] == "identical":
        # the three deviations are roots of ~1e-16 of rounding left by a full cancellation (every similarity is 1): compared in the
        # radicand, relative to the terms that cancel (E[g^2] = 1; for mdsi the deviation sum itself is what finish receives)
        assert bool(((got[:, 0] ** 2 - want[:, 0] ** 2).abs() <= 1e-12).all()) and bool(((got[:, 1] ** 2 - want[:, 1] ** 2).abs() <= 1e-12).all())
        cols = (2, 3, 4, 5)
    else:
        cols = range(6)
    for k in cols:
        err = (got[:, k] - want[:, k]).abs()
        print(f"{_id(case)} finish out[{k}] {got[:, k].tolist()} max rel {float((err / want[:, k].abs().clamp_min(1e-300)).max()):.2e}")
        assert bool((err <= 1e-12 * want[:, k].abs()).all()), (k, got[:, k], want[:, k])
        _note(f"finish[{k}]", float((err / want[:, k].abs().clamp_min(1e-300)).max()), 1e-12, case)


@pytest.mark.parametrize("case", MDSI_CASES, ids=_id)
def test_mdsi_kernel_sizes(engine, case):
    """min side / 256 = 0.5, 1.5, 2.5, 3.5 (Python's round: ties to even -> k = 1, 2, 2, 4) and 641 -> k = 3 (pad 1 left, 1 right)"""
    c, e = reference(case, True), engine_results(engine, case, True)
    H, W = case[1]
    k = {128: 1, 384: 2, 640: 2, 641: 3, 896: 4}[H]
    assert E.mdsi_kernel_size(H, W) == k and e["stage"]["m"][1]["h"] == (H - 1) // k + 1 == c["r64"]["m"][0].shape[1]
    check_images(e, c, case, ("m",))
    check_partials(e, c, case, ("mdsi1", "mdsi2"))
    check_accumulated(e, c, case, True)
    a = accumulated_from_partials(e, True)
    assert bool(((e["out"][:, 3] - a["mdsi_dev"] ** 0.25).abs() <= 1e-12 * e["out"][:, 3].abs()).all())
    one = run(engine, c["p"][1:2], c["t"][1:2], MDSI_REGIONS)
    assert torch.equal(one["out"][0, 3], e["out"][1, 3])
    assert torch.equal(one["stage"]["mdsi2"][0][0], e["stage"]["mdsi2"][0][1])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_middle_image_of_three_is_its_own_batch_of_one_bitwise(engine, case):
    c, e = reference(case), engine_results(engine, case)
    one = run(engine, c["p"][1:2], c["t"][1:2])
    assert torch.equal(one["out"][0], e["out"][1])
    for name in IMAGES:
        for side in (0, 1):
            assert torch.equal(one["stage"][name][0][side][0], e["stage"][name][0][side][1]), (name, side)
    for name in PARTIALS:
        assert torch.equal(one["stage"][name][0][0], e["stage"][name][0][1]), name
        assert {k: v for k, v in one["stage"][name][1].items() if k != "B"} == {k: v for k, v in e["stage"][name][1].items() if k != "B"}


def test_flat_zero_background_windows_give_exactly_zero(engine):
    """a VIF window over nothing but zero background has no variance in either image: both of its terms are exactly 0, wherever the
    window's tile starts; so a tile of such windows sums to exactly 0"""
    H = W = 80
    t = torch.zeros((1, H, W))
    t[0, 0, 0] = 0.9                      # the first pixel of the first tile: what a tile-wide origin would be taken from
    t[0, 64:, 64:] = 0.5
    p = t.clone()
    p[0, 70, 70] = 0.7
    e = run(engine, p, t)
    part, info = e["stage"]["vif0"]
    r64 = E.vif_maps(p.double(), t.double())[0]
    num, den = E.tile_sums(r64[2], 16, 16)[0], E.tile_sums(r64[3], 16, 16)[0]
    assert info["tiles_x"] == 4 and info["ntiles"] == 16
    flat = [i for i in range(16) if float(den[i]) == 0.0 and float(num[i]) == 0.0]
    assert 1 in flat and 5 in flat and len(flat) >= 6, flat           # tiles whose every window sees zeros only
    print("vif0 partials of the all-zero tiles:", part[0, flat].tolist())
    assert bool((part[0, flat] == 0).all()), part[0, flat]
    # tile 0 holds the windows over the lone source and, from row / column 1 on, windows over zeros only: per window that cannot be read
    # back, but the tile's sum must be the source's windows alone
    assert abs(float(part[0, 0, 1]) - float(den[0])) <= 5e-6 and abs(float(part[0, 0, 0]) - float(num[0])) <= 5e-6


@pytest.mark.parametrize("where", ["preds", "target"])
@pytest.mark.parametrize("at", [(30, 17), (16, 16), (0, 0), (60, 52)])
def test_nan_pixel_reaches_exactly_its_support(engine, where, at):
    case = ("photon", (61, 53))
    c, clean = reference(case), engine_results(engine, case)
    p, t = c["p"].clone(), c["t"].clone()
    (p if where == "preds" else t)[1, at[0], at[1]] = float("nan")
    want = ref_maps(p.double(), t.double())
    nan = torch.full_like(p, float("nan")).to(DEV)
    engine.eval(nan, nan)
    out = engine.eval(p.to(DEV), t.to(DEV)).cpu()
    for name in IMAGES:
        for side in (0, 1):
            g = engine.stage(name, side)[0].cpu()
            assert torch.equal(torch.isnan(g), torch.isnan(want[name][side])), (name, side)
            assert torch.equal(g[[0, 2]], clean["stage"][name][0][side][[0, 2]]), (name, side)
    for name in PARTIALS:
        part, info = engine.stage(name)
        part = part.cpu()
        assert torch.equal(part[[0, 2]], clean["stage"][name][0][[0, 2]]), name
        for k, m in enumerate(want[name]):
            exp = torch.isnan(E.tile_sums(m, info["tile_h"], info["tile_w"]))
            assert torch.equal(torch.isnan(part[:, :, k]), exp), (name, k, torch.isnan(part[1, :, k]).nonzero().flatten().tolist(), exp[1].nonzero().flatten().tolist())
            if name in ("haar", "mdsi1", "mdsi2") or name == "gms0" and k < 2 or name == "vif0" and (k == 0 or where == "target"):
                assert bool(exp[1].any()), (name, k)          # the reference does see it (VIF's decimation can drop the last row / column)
    assert torch.equal(out[[0, 2]], clean["out"][[0, 2]])
    a = accumulated_from_maps(want)
    ref_nan = torch.stack([a["gmsd_dev"], sum(a[f"ms_gmsd_dev{k}"] for k in range(4)), a["haar_num"] + a["haar_den"], a["mdsi_dev"], a["vif_num"], a["vif_den"]], 1)
    assert torch.equal(torch.isnan(out), torch.isnan(ref_nan)), (out, ref_nan)
    assert bool(torch.isnan(out[1, :5]).all()) and bool(torch.isnan(out[1, 4] / out[1, 5]))          # every metric of that image


def test_stage_refusals(engine):
    from xmm_superres_denoise.engine import ExtMetricsEngine, XsdError, _lib
    L = _lib.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    info = (ctypes.c_int32 * 8)()
    buf = torch.zeros(1 << 16, device=DEV)
    z = torch.zeros((1, 64, 64), device=DEV)
    with torch.cuda.device(DEV):
        fresh = ExtMetricsEngine()
    assert L.xsd_ext_metrics_test_stage(fresh.h, 0, 0, buf.data_ptr(), buf.numel() * 4, info, stream) == -1
    assert b"has not evaluated" in L.xsd_last_error()
    with pytest.raises(XsdError, match="has not evaluated"):
        fresh.stage("u1")
    fresh.eval(z, z)
    ok = (fresh.h, 0, 0, buf.data_ptr(), buf.numel() * 4, info, stream)
    assert L.xsd_ext_metrics_test_stage(*ok) == 0 and list(info)[:4] == [1, 32, 32, 0]
    for i in (0, 3, 5):
        args = list(ok)
        args[i] = None
        assert L.xsd_ext_metrics_test_stage(*args) == -1
        assert b"null pointer" in L.xsd_last_error()
    for stage in (-1, len(ExtMetricsEngine.STAGES)):
        assert L.xsd_ext_metrics_test_stage(fresh.h, stage, 0, buf.data_ptr(), buf.numel() * 4, info, stream) == -1
        assert b"unknown stage" in L.xsd_last_error()
    assert L.xsd_ext_metrics_test_stage(fresh.h, 0, 2, buf.data_ptr(), buf.numel() * 4, info, stream) == -1
    assert b"side must be" in L.xsd_last_error()
    for name in ExtMetricsEngine.STAGES:
        s = ExtMetricsEngine.STAGES.index(name)
        full, _ = fresh.stage(name)
        need = full.numel() * full.element_size()
        buf.fill_(7.0)
        assert L.xsd_ext_metrics_test_stage(fresh.h, s, 0, buf.data_ptr(), need - 1, info, stream) == -1
        assert b"buffer too small" in L.xsd_last_error() and str(need).encode() in L.xsd_last_error()
        assert L.xsd_ext_metrics_test_stage(fresh.h, s, 0, buf.data_ptr(), -1, info, stream) == -1
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all())                               # a refused call copies nothing
        assert L.xsd_ext_metrics_test_stage(fresh.h, s, 0, buf.data_ptr(), need, info, stream) == 0
    with pytest.raises(XsdError, match="unknown stage"):
        fresh.stage("u4")
    with pytest.raises(XsdError, match="float32"):
        fresh.stage("gms0", out=torch.zeros(4096, device=DEV))        # partials are doubles
    torch.cuda.synchronize()


def test_zz_worst_error_over_bar_per_stage():
    """not a check of its own: prints the table DESIGN.md section 24 quotes (every figure was asserted <= 1 where it was measured)"""
    for stage in sorted(WORST):
        print(f"WORST {stage:16s} error/bar {WORST[stage][0]:.3f}  at {WORST[stage][1]}")
