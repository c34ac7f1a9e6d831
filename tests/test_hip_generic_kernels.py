"""The generic-width kernels one by one (csrc/generic_net.hip) through xsd_test_gconv / xsd_test_gwgrad / xsd_test_gop / xsd_test_gpack: a
GenericNet that is ONE conv, packed by the net's own pack() and launched by the net's own conv() / wgrad() / ew(), dispatch included.

Reference: torch.nn.functional.conv2d plus the GConvP epilogue written out, float64 on the CPU; input gradients, weight gradients and the
unshuffle against autograd (through conv2d, pixel_shuffle, leaky_relu).
Bars: outputs max|got - ref| <= 2e-5 max|ref| per tensor, dw / db 5e-5 (the single-kernel bars of test_hip_kernels.py for exact-fp32
kernels: fmaf chains of K = 9 cin <= 720 terms here).  Selects, clamps and the packed buffers compare bits.
Every tensor of a launch lies between NaN guard bands in one allocation.  Inputs are channel views of larger tensors whose other channels
hold NaN (the dense block's slab: the buffer descriptor's range check must keep them out), outputs start as NaN, and everything a launch
does not own -- other slab channels, batch-stride gaps, the rest of the flat gradient buffer -- must keep its bits."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util_hip import Guarded

pytestmark = pytest.mark.gpu

TOL, TOL_DW = 2e-5, 5e-5
DIRECT, MFMA = 1, 2
WORST = {}
DISTINCT = dict(a1=0.7, s1=0.75, a2=0.3, s2=-1.25, slope=0.2)      # with a non-trivial bias and e1c < cout: seven distinct quantities
TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def L():
    from xmm_superres_denoise.engine import _lib
    return _lib.load()


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def f32(v):
    return float(np.float32(v))


def assert_close(got, ref, family, what="", tol=TOL):
    """max|got - ref| <= tol max|ref| over the finite entries of ref; its non-finite entries (planted inf / NaN) must match exactly"""
    nf = ~np.isfinite(ref)
    if nf.any():
        assert np.array_equal(got[nf], ref[nf].astype(np.float32), equal_nan=True), f"{family} {what}: a planted inf / NaN came back differently"
        got, ref = np.where(nf, 0, got), np.where(nf, 0, ref)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    rel = err / (scale + 1e-300)
    WORST[family] = max(WORST.get(family, 0.0), rel)
    print(f"{family} {what}: max|got - ref| {err:.3e} = {rel:.2e} of max|ref| {scale:.3e} (worst so far {WORST[family]:.2e})")
    assert err <= tol * scale, f"{family} {what}: {err:.3e} > {tol * scale:.3e}"


def view(g, spec):
    """(tensor name, first channel) -> (device pointer, batch stride in floats) of a channel view of a [B, C, H, W] tensor"""
    if spec is None:
        return None, 0
    name, ch = spec
    t = g.t[name]
    hw = t.shape[2] * t.shape[3]
    return g.ptr(name, ch * hw), t.shape[1] * hw


def nan_nchw(B, C, H, W):
    return np.full((B, C, H, W), np.nan, np.float32)


def make_wb(rng, cout, cin):
    return (rng.normal(size=(cout, cin, 3, 3)) / np.sqrt(9.0 * cin)).astype(np.float32), rng.normal(size=cout).astype(np.float32)


def flat_params(w, b, off):
    return np.concatenate([np.full(off, np.nan, np.float32), w.reshape(-1), b, np.full(5, np.nan, np.float32)])


# =====================================================================================================================================
# convs
# =====================================================================================================================================

def check_conv(L, cout, cin, shape, seed, layout="slab", transposed=False, w=None, b=None, x=None, expect_path=None, param_off=0,
               e1=False, e1c=None, e2=None, skip=None, pre=False, family=None, what="", **ep):
    """One conv launch against float64.  layout "slab": x = the first channels of a [B][ci + co + 3][H][W] tensor, y = the next co channels,
    NaN everywhere else; "slab5": the dense block's own [B][5 nf][H][W] with nf = co and ci = k nf; "gap": x = channels 1 .. ci of a
    [B][ci + 2] tensor, y = channels 0 .. co - 1 of a [B][co + 1] tensor (forced with shuffle); "prefix": like gap for x, y = the first co
    channels of a [B][co + 2] tensor.  e1 / e2 / skip: True or data; skip "one" = one broadcast channel.  Returns (y, pre, path)."""
    from xmm_superres_denoise.engine._lib import XsdTestGconvArgs
    B, H, W = shape
    rng = np.random.default_rng(seed)
    co, ci = (cin, cout) if transposed else (cout, cin)          # the launched conv's output / input channel counts
    if w is None:
        w, b0 = make_wb(rng, cout, cin)
        b = b0 if b is None else b
    if x is None:
        x = rng.normal(size=(B, ci, H, W)).astype(np.float32)
    shuffle, accumulate = int(ep.get("shuffle", 0)), int(ep.get("accumulate", 0))
    if shuffle:
        layout = "gap"
    items = dict(params=flat_params(w, b, param_off))
    if layout in ("slab", "slab5"):
        ctot = 5 * co if layout == "slab5" else ci + co + 3
        assert ci + co <= ctot and (layout == "slab" or ci % co == 0)
        cont = nan_nchw(B, ctot, H, W)
        cont[:, :ci] = x
        xspec, yspec, ycont = ("slab", 0), ("slab", ci), "slab"
        items["slab"] = cont
    else:
        xc = nan_nchw(B, ci + 2, H, W)
        xc[:, 1:1 + ci] = x
        items["xc"] = xc
        xspec, yspec, ycont = ("xc", 1), ("yc", 0), "yc"
        cont = nan_nchw(B, co // 4 + 1, 2 * H, 2 * W) if shuffle else nan_nchw(B, co + (2 if layout == "prefix" else 1), H, W)
        items["yc"] = cont
    ych, yn = yspec[1], (co // 4 if shuffle else co)
    y0 = None
    if accumulate:
        y0 = rng.normal(size=cont[:, ych:ych + yn].shape).astype(np.float32)
        cont[:, ych:ych + yn] = y0
    if pre:
        items["prec"] = np.full(cont.shape, np.nan, np.float32)
    e1c = co if e1c is None else e1c
    if e1 is not False:
        e1 = rng.normal(size=(B, co, H, W)).astype(np.float32) if e1 is True else e1
        c = nan_nchw(B, co + 1, H, W)
        c[:, :e1c] = e1[:, :e1c]                                 # channels >= e1c hold NaN: the kernel must not read them
        items["e1"] = c
    if e2 is not None:
        e2 = rng.normal(size=(B, co, H, W)).astype(np.float32) if e2 is True else e2
        c = nan_nchw(B, co + 1, H, W)
        c[:, :co] = e2
        items["e2"] = c
    skipc = 0
    if skip is not None:
        if isinstance(skip, str):
            skip = rng.uniform(size=(B, 1 if skip == "one" else co, H, W)).astype(np.float32)
        skipc = skip.shape[1]
        c = nan_nchw(B, skipc + 2, H, W)
        c[:, 1:1 + skipc] = skip
        items["skip"] = c
    g = Guarded(ro=[k for k in items if k not in (ycont, "prec")], **items)
    a = XsdTestGconvArgs()
    a.x, a.xbs = view(g, xspec)
    a.y, a.ybs = view(g, yspec)
    a.a1, a.a2, a.slope = ep.get("a1", 1.0), ep.get("a2", 1.0), ep.get("slope", 1.0)
    a.s1, a.s2 = ep.get("s1", 1.0), ep.get("s2", 1.0)
    a.e1, a.e1bs = view(g, ("e1", 0) if "e1" in items else None)
    a.e1c = e1c
    a.e2, a.e2bs = view(g, ("e2", 0) if "e2" in items else None)
    a.skip, a.skipbs = view(g, ("skip", 1) if "skip" in items else None)
    a.skipc = skipc
    a.pre = view(g, ("prec", ych))[0] if pre else None
    a.accumulate, a.shuffle, a.clamp01 = accumulate, shuffle, int(ep.get("clamp01", 0))
    path = ctypes.c_int(0)
    rc = L.xsd_test_gconv(cout, cin, g.ptr("params"), param_off, int(transposed), ctypes.byref(a), B, H, W, ctypes.byref(path), None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.xsd_last_error().decode())
    assert expect_path is None or path.value == expect_path, f"ran path {path.value}, meant {expect_path}"
    g.check()
    # ---- float64 reference ----
    wt, xt = torch.from_numpy(w).double(), torch.from_numpy(x).double()
    if transposed:
        X = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
        v, = torch.autograd.grad(F.conv2d(X, wt, padding=1), X, xt)
    else:
        v = F.conv2d(xt, wt, torch.from_numpy(b).double(), padding=1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = v.numpy() * f32(a.a1)
        if "e1" in items:
            v[:, :e1c] += f32(a.s1) * e1[:, :e1c].astype(np.float64)
        v = v * f32(a.a2)
        if "e2" in items:
            v = v + f32(a.s2) * e2.astype(np.float64)
        v = np.where(v > 0, v, v * f32(a.slope))
        if skip is not None:
            v = v + skip.astype(np.float64)
        if shuffle:
            v = F.pixel_shuffle(torch.from_numpy(v), 2).numpy()
        if accumulate:
            v = v + y0.astype(np.float64)
        ref_pre = v
        ref_y = torch.from_numpy(v).clamp(0, 1).numpy() if a.clamp01 else v
    family = family or ("gconv_mfma" if path.value == MFMA else "gconv3x3")
    outs = []
    for name, ref in ((ycont, ref_y), ("prec", ref_pre)):
        if name not in g.t:
            outs.append(None)
            continue
        got, before = g.np(name), g.before[name].cpu().numpy()
        owned = np.zeros(got.shape, bool)
        owned[:, ych:ych + yn] = True
        assert np.array_equal(got.view(np.uint32)[~owned], before.view(np.uint32)[~owned]), f"{name}: an element the launch does not own changed"
        part = got[:, ych:ych + yn]
        assert np.array_equal(np.isnan(part), np.isnan(ref)), f"{name}: an element was not written (or a NaN leaked in)"
        assert_close(part, ref, family, f"{what} ({cout},{cin}) {shape} {layout}{' T' if transposed else ''} {name}")
        outs.append(part)
    return outs[0], outs[1], path.value


def test_dispatch(L):
    """at least 16 channels on BOTH sides: the matrix instruction; one short on either side: direct.  All three against the same reference."""
    for (cout, cin), path in (((16, 16), MFMA), ((15, 16), DIRECT), ((16, 15), DIRECT)):
        check_conv(L, cout, cin, (2, 19, 21), 11, expect_path=path, slope=0.2)
        check_conv(L, cout, cin, (2, 19, 21), 12, transposed=True, expect_path=path)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 19, 21), (1, 16, 16), (1, 17, 33)])
@pytest.mark.parametrize("cc", [(1, 1), (3, 9), (10, 8), (8, 10), (9, 12)])
def test_direct_conv(L, cc, shape):
    """16 x 16 tiles, 8 output channels per thread, 8 input channels per round: channel counts below, at and above 8, shapes at and around the tile"""
    check_conv(L, cc[0], cc[1], shape, seed_of(cc, shape), expect_path=DIRECT, slope=0.2)


@pytest.mark.parametrize("shape", [(1, 8, 32), (2, 19, 45), (1, 9, 33), (3, 5, 7)])
@pytest.mark.parametrize("cc", [(16, 16), (20, 20), (36, 20), (20, 36), (32, 64), (33, 80)])
def test_mfma_conv(L, cc, shape):
    """8 x 32 tiles, 32-channel blocks: channel counts below, at and above one and two blocks.  x is a slab prefix with NaN in every channel
    past cin: a range check that lets one channel past cin through turns the whole output NaN."""
    check_conv(L, cc[0], cc[1], shape, seed_of(cc, shape), expect_path=MFMA, slope=0.2)


@pytest.mark.parametrize("nf,k,path", [(16, 1, MFMA), (20, 1, MFMA), (20, 4, MFMA), (32, 2, MFMA), (8, 2, DIRECT), (8, 4, DIRECT)])
def test_dense_block_slab(L, nf, k, path):
    """exactly how the dense block launches: x = channels [0, k nf) of [B][5 nf][H][W] (xbs = 5 nf H W), y = the next nf channels, NaN past cin"""
    check_conv(L, nf, k * nf, (2, 19, 45), 70 + nf + k, layout="slab5", expect_path=path, slope=0.2)


@pytest.mark.parametrize("cc", [(9, 12), (36, 20)])
@pytest.mark.parametrize("form", ["distinct", "engine_slope", "engine_e1", "engine_e1_e2", "accumulate"])
def test_epilogue(L, cc, form):
    """seven distinct quantities (a swap of any two shows far above the bar; channels >= e1c of e1 hold NaN); the engine's own three settings
    (a dense conv, a dense block's last conv, an RRDB's last conv); accumulate onto a random tensor"""
    cout, cin = cc
    kw = dict(distinct=dict(e1=True, e1c=cout - 3, e2=True, **DISTINCT), engine_slope=dict(slope=0.2), engine_e1=dict(a1=0.2, e1=True, s1=1.0),
              engine_e1_e2=dict(a1=0.2, e1=True, s1=1.0, a2=0.2, e2=True, s2=1.0), accumulate=dict(accumulate=1, slope=0.2))[form]
    check_conv(L, cout, cin, (2, 19, 45), seed_of(cc, form), layout="gap", what=form, **kw)
    check_conv(L, cout, cin, (1, 9, 33), seed_of(cc, form, 2), layout="slab", what=form, **kw)


@pytest.mark.parametrize("cout,cin", [(16, 4), (16, 16), (80, 20)])
def test_shuffle(L, cout, cin):
    """the upsample conv's store addressing against pixel_shuffle of the float64 conv, LeakyReLU(0.01); the batch-stride gap keeps its NaN"""
    check_conv(L, cout, cin, (2, 9, 13), 90 + cout, shuffle=1, slope=0.01, what="shuffle")


@pytest.mark.parametrize("cc", [(3, 20), (20, 20)])
@pytest.mark.parametrize("bcast", ["full", "one"])
def test_head_skip_pre_clamp(L, cc, bcast):
    """the DN head: skip with skipc = cout and with one broadcast channel, pre returned next to the clamped y"""
    y, pre, _ = check_conv(L, cc[0], cc[1], (2, 19, 45), seed_of(cc, bcast), layout="gap", skip=bcast, pre=True, clamp01=1, what=f"head {bcast}")
    assert np.array_equal(y, np.clip(pre, 0, 1)) and (pre < 0).any() and (pre > 1).any()


@pytest.mark.parametrize("cc", [(3, 9), (20, 20)])
def test_clamp_at_the_bounds(L, cc):
    """zero weights and bias: the value is the skip operand exactly.  0, 1, -0.0 stay, +-inf go to the bounds, NaN reaches y as NaN"""
    cout, cin = cc
    B, H, W = 1, 5, 40
    specials = np.array([0.0, 1.0, -0.0, np.inf, -np.inf, np.nan, -TINY, np.nextafter(np.float32(1), np.float32(2)), 0.5, 1e-45], np.float32)
    skip = np.full((B, cout, H, W), 0.25, np.float32)
    for c in range(cout):
        skip[0, c, c % H, 3:3 + len(specials)] = specials
    y, pre, _ = check_conv(L, cout, cin, (B, H, W), 5, layout="gap", w=np.zeros((cout, cin, 3, 3), np.float32), b=np.zeros(cout, np.float32),
                           skip=skip, pre=True, clamp01=1, what="clamp specials")
    want_pre = (np.float32(0.0) + skip).astype(np.float32)
    assert np.array_equal(pre.view(np.uint32), want_pre.view(np.uint32))
    want = torch.from_numpy(want_pre).clamp(0, 1).numpy()
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and np.isnan(y).sum() == cout


@pytest.mark.parametrize("cc", [(3, 9), (20, 20)])
@pytest.mark.parametrize("via", ["bias", "e2"])
def test_lrelu_select_at_zero(L, cc, via):
    """v > 0 keeps, everything else takes the slope -- here -2, so that a zero that wrongly `keeps` shows in its sign bit: +0.0 and -0.0 come
    out as -0.0, the smallest subnormal stays, -tiny doubles.  Zero weights; the value is planted through the bias (per channel) or e2."""
    cout, cin = cc
    B, H, W = 2, 5, 9
    specials = np.array([0.0, -0.0, 1e-45, -TINY], np.float32)
    zw = np.zeros((cout, cin, 3, 3), np.float32)
    if via == "bias":
        b = specials[np.arange(cout) % 4]
        y, _, _ = check_conv(L, cout, cin, (B, H, W), 6, layout="gap", w=zw, b=b, slope=-2.0, what="select via bias")
        v = np.broadcast_to((np.float32(0.0) + b)[None, :, None, None], y.shape)
    else:
        e2 = specials[np.arange(B * cout * H * W) % 4].reshape(B, cout, H, W)
        y, _, _ = check_conv(L, cout, cin, (B, H, W), 6, layout="gap", w=zw, b=np.zeros(cout, np.float32), e2=e2, slope=-2.0, what="select via e2")
        v = np.float32(0.0) + e2
    want = np.where(v > 0, v, v * np.float32(-2.0)).astype(np.float32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert (want.view(np.uint32) == 0x80000000).any() and (want.view(np.uint32) == 1).any()


@pytest.mark.parametrize("cc", [(3, 9), (36, 20), (20, 36)])
@pytest.mark.parametrize("shape", [(2, 19, 45), (1, 9, 33)])
def test_transposed_conv(L, cc, shape):
    """gpack_kernel -> direct kernel and gpack_blocks_kernel z = 1 -> matrix kernel against autograd dL/dx; asymmetric channel counts, so a
    swapped index cannot cancel.  Once plain, once accumulating into a slab prefix (the dense block's backward)."""
    path = MFMA if min(cc) >= 16 else DIRECT
    check_conv(L, cc[0], cc[1], shape, seed_of(cc, shape), transposed=True, expect_path=path, param_off=37)
    check_conv(L, cc[0], cc[1], shape, seed_of(cc, shape, 1), transposed=True, expect_path=path, layout="prefix", accumulate=1)


# =====================================================================================================================================
# weight gradients
# =====================================================================================================================================

def check_wgrad(L, cout, cin, shape, seed, expect_path, expect_parts, param_off=37):
    B, H, W = shape
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, cin, H, W)).astype(np.float32)
    gy = rng.normal(size=(B, cout, H, W)).astype(np.float32)
    xs = nan_nchw(B, cin + cout + 3, H, W)
    xs[:, :cin] = x
    gs = nan_nchw(B, cout + 5, H, W)
    gs[:, 2:2 + cout] = gy
    n = cout * cin * 9
    total = param_off + n + cout + 50
    g = Guarded(ro=("xs", "gs"), xs=xs, gs=gs, grads=(total,), grads2=(total,))
    res = []
    for name in ("grads", "grads2"):
        path, parts = ctypes.c_int(0), ctypes.c_int(0)
        xp, xbs = view(g, ("xs", 0))
        gp, gbs = view(g, ("gs", 2))
        assert gbs != cout * H * W
        rc = L.xsd_test_gwgrad(cout, cin, param_off, xp, xbs, gp, gbs, g.ptr(name), B, H, W, ctypes.byref(path), ctypes.byref(parts), None)
        torch.cuda.synchronize()
        assert rc == 0, (rc, L.xsd_last_error().decode())
        assert (path.value, parts.value) == (expect_path, expect_parts), f"ran path {path.value} with {parts.value} parts"
        res.append(g.np(name))
    g.check()
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32)), "two runs differ"
    flat = res[0]
    assert np.isnan(flat[:param_off]).all() and np.isnan(flat[param_off + n + cout:]).all(), "the rest of the flat gradient buffer was written"
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    dw, db = torch.autograd.grad(F.conv2d(torch.from_numpy(x).double(), wt, bt, padding=1), (wt, bt), torch.from_numpy(gy).double())
    family = "gwgrad_mfma" if expect_path == MFMA else "gwgrad_direct"
    assert_close(flat[param_off:param_off + n].reshape(cout, cin, 3, 3), dw.numpy(), family, f"dw ({cout},{cin}) {shape} parts {expect_parts}", TOL_DW)
    assert_close(flat[param_off + n:param_off + n + cout], db.numpy(), family, f"db ({cout},{cin}) {shape}", TOL_DW)


@pytest.mark.parametrize("shape,parts", [((2, 19, 45), 3), ((1, 8, 32), 1)])
@pytest.mark.parametrize("cc", [(16, 16), (36, 20), (20, 80)])
def test_wgrad_mfma(L, cc, shape, parts):
    """(2, 19, 45) is 12 tiles of 8 x 32: three parts of four tiles each; (1, 8, 32) one tile, one part.  x a slab prefix with NaN past cin,
    g a channel view of a wider tensor (gbs != cout H W) with NaN around it."""
    check_wgrad(L, cc[0], cc[1], shape, seed_of(cc, shape), MFMA, parts)


@pytest.mark.parametrize("shape,parts", [((3, 5, 7), 1), ((1, 70, 61), 2)])
@pytest.mark.parametrize("cc", [(3, 9), (10, 1), (1, 12)])
def test_wgrad_direct(L, cc, shape, parts):
    """(1, 70, 61) = 4270 pixels: two parts of 2135, which the 256-thread sweep leaves ragged (2135 = 8 * 256 + 87)"""
    check_wgrad(L, cc[0], cc[1], shape, seed_of(cc, shape), DIRECT, parts)


# =====================================================================================================================================
# packers
# =====================================================================================================================================

def blocks_of(wk):
    """[co][ci][9] -> [co blk][ci blk][tap][32 ci][32 co], zero-padded"""
    co, ci, _ = wk.shape
    nco, nci = (co + 31) // 32, (ci + 31) // 32
    p = np.zeros((nco * 32, nci * 32, 9), np.float32)
    p[:co, :ci] = wk
    return np.ascontiguousarray(p.reshape(nco, 32, nci, 32, 9).transpose(0, 2, 4, 3, 1))


def test_packers(L):
    """wt = [ci][co][8 - t] per conv; wblk = both z forms of gpack_blocks_kernel per wide conv: the conv itself and its input-gradient conv
    (W^T with flipped taps), zero-padded.  The narrow conv between the two wide ones has pf = pt = -1 and must write nothing: wblk is
    exactly the wide convs' blocks, so a stray element lands in one of them."""
    table = [(36, 20), (3, 9), (16, 33)]
    rng = np.random.default_rng(8)
    ws = [make_wb(rng, co, ci) for co, ci in table]
    params = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in ws])
    wt_n = sum(co * ci * 9 for co, ci in table)
    wb_n = sum(2 * ((co + 31) // 32) * ((ci + 31) // 32) * 9 * 1024 for co, ci in table if min(co, ci) >= 16)
    g = Guarded(ro=("params",), params=params, wt=(wt_n,), wblk=(wb_n,))
    couts, cins = (ctypes.c_int * 3)(*[t[0] for t in table]), (ctypes.c_int * 3)(*[t[1] for t in table])
    off, cnt = (ctypes.c_int64 * 9)(), (ctypes.c_int64 * 2)()
    rc = L.xsd_test_gpack(3, couts, cins, g.ptr("params"), g.ptr("wt"), wt_n, g.ptr("wblk"), wb_n, off, cnt, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.xsd_last_error().decode())
    g.check()
    assert list(cnt) == [wt_n, wb_n] and list(off)[3:6] == [36 * 20 * 9, -1, -1]
    wt, wblk = g.np("wt"), g.np("wblk")
    want_blk = np.full(wb_n, np.nan, np.float32)
    for i, ((co, ci), (w, _)) in enumerate(zip(table, ws)):
        wk = w.reshape(co, ci, 9)
        want = np.ascontiguousarray(wk.transpose(1, 0, 2)[:, :, ::-1]).reshape(-1)
        t, pf, pt = off[3 * i], off[3 * i + 1], off[3 * i + 2]
        assert np.array_equal(wt[t:t + want.size].view(np.uint32), want.view(np.uint32)), f"wt of conv {i}"
        if pf >= 0:
            fwd = blocks_of(wk).reshape(-1)
            bwd = blocks_of(np.ascontiguousarray(wk.transpose(1, 0, 2)[:, :, ::-1])).reshape(-1)
            want_blk[pf:pf + fwd.size] = fwd
            want_blk[pt:pt + bwd.size] = bwd
    assert np.array_equal(wblk.view(np.uint32), want_blk.view(np.uint32)), "wblk != the numpy block transpose"


# =====================================================================================================================================
# elementwise kernels
# =====================================================================================================================================

def gop(L, op, g, d, s, s2, B, C, H, W, a):
    dp, dbs = view(g, d)
    sp, sbs = view(g, s)
    rc = L.xsd_test_gop(op, dp, dbs, sp, sbs, view(g, s2)[0], B, C, H, W, a, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.xsd_last_error().decode())
    g.check()


EW = (2, 5, 5, 7)      # B, C, H, W: HW = 35


@pytest.mark.parametrize("op", [0, 1, 2])
def test_gew(L, op):
    """copy * a, axpy, d *= lrelu'(s): d and s are channel views with different batch strides, neither C H W; the gaps keep their NaN.
    op 2 decides at s = +0.0, -0.0, the smallest subnormal, -tiny (bit compare: a select)."""
    B, C, H, W = EW
    rng = np.random.default_rng(20 + op)
    d0, s = rng.normal(size=EW).astype(np.float32), rng.normal(size=EW).astype(np.float32)
    if op == 2:
        s.reshape(-1)[::3] = np.array([0.0, -0.0, 1e-45, -TINY], np.float32)[np.arange(len(s.reshape(-1)[::3])) % 4]
    dc, sc = nan_nchw(B, C + 2, H, W), nan_nchw(B, C + 3, H, W)
    dc[:, 1:1 + C] = d0 if op else np.nan
    sc[:, 2:2 + C] = s
    g = Guarded(ro=("sc",), dc=dc, sc=sc)
    a = np.float32(0.3)
    gop(L, op, g, ("dc", 1), ("sc", 2), None, B, C, H, W, float(a))
    got = g.np("dc")
    assert np.isnan(got[:, [0, C + 1]]).all(), "a batch-stride gap was written"
    want = (a * s, d0 + a * s, np.where(s > 0, d0, d0 * a))[op].astype(np.float32)
    if op == 1:
        assert_close(got[:, 1:1 + C], d0.astype(np.float64) + f32(a) * s.astype(np.float64), "gew", "axpy")
    else:
        assert np.array_equal(got[:, 1:1 + C].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("C4", [8, 20])
def test_gunshuffle(L, C4):
    """against autograd of leaky_relu(pixel_shuffle(.), 0.01); U holds +-0.0 (no gradient passes at zero: the slope applies)"""
    B, H, W = 2, 5, 7
    rng = np.random.default_rng(30 + C4)
    conv_out = rng.normal(size=(B, C4, H, W)).astype(np.float32)
    conv_out.reshape(-1)[::5] = np.array([0.0, -0.0], np.float32)[np.arange(len(conv_out.reshape(-1)[::5])) % 2]
    dU = rng.normal(size=(B, C4 // 4, 2 * H, 2 * W)).astype(np.float32)
    U = F.pixel_shuffle(torch.from_numpy(conv_out), 2).numpy()
    g = Guarded(ro=("dU", "U"), dU=dU, U=U, G=(B, C4, H, W))
    gop(L, 3, g, ("G", 0), ("dU", 0), ("U", 0), B, C4, H, W, 0.01)
    # the engine stores U = lrelu(shuffle(conv)): its sign is the conv's, and lrelu'(0) = slope in torch as in the kernel
    c = torch.from_numpy(conv_out).double().requires_grad_(True)
    ref, = torch.autograd.grad(F.leaky_relu(F.pixel_shuffle(c, 2), 0.01), c, torch.from_numpy(dU).double())
    got = g.np("G")
    assert_close(got, ref.numpy(), "gew", f"unshuffle C4 {C4}")
    sel = F.pixel_unshuffle(torch.from_numpy(np.where(U > 0, dU, dU * np.float32(0.01)).astype(np.float32)), 2).numpy()
    assert np.array_equal(got.view(np.uint32), sel.view(np.uint32)), "the select is not bit-exact"


def test_gsum_channels(L):
    B, C, HW = 2, 3, 35
    rng = np.random.default_rng(40)
    d0, s = rng.normal(size=(B, 1, 5, 7)).astype(np.float32), rng.normal(size=(B, C, 5, 7)).astype(np.float32)
    g = Guarded(ro=("s",), d=d0, s=s)
    gop(L, 4, g, ("d", 0), ("s", 0), None, B, C, 5, 7, 0.0)
    assert_close(g.np("d"), d0.astype(np.float64) + s.astype(np.float64).sum(axis=1, keepdims=True), "gew", "sum_channels")


def test_gclamp_bwd(L):
    """the gradient passes iff 0 <= pre <= 1 (bounds included, like torch.clamp); NaN and +-inf block it"""
    pre = np.array([-TINY, -0.0, 0.0, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.nan, np.inf, -np.inf, 1e-45], np.float32)
    passes = np.array([0, 1, 1, 1, 1, 0, 0, 0, 0, 1], bool)
    n = 70
    pre = np.resize(pre, n).reshape(2, 1, 5, 7)
    dy = np.random.default_rng(41).normal(size=pre.shape).astype(np.float32)
    g = Guarded(ro=("pre", "dy"), pre=pre, dy=dy, d=pre.shape)
    gop(L, 5, g, ("d", 0), ("pre", 0), ("dy", 0), 2, 1, 5, 7, 0.0)
    want = np.where(np.resize(passes, n).reshape(pre.shape), dy, np.float32(0.0))
    assert np.array_equal(g.np("d").view(np.uint32), want.view(np.uint32))
    x = torch.from_numpy(np.nan_to_num(pre, nan=2.0)).double().requires_grad_(True)      # torch agrees on every non-NaN entry
    tg, = torch.autograd.grad(x.clamp(0, 1), x, torch.from_numpy(dy).double())
    assert np.array_equal(tg.numpy().astype(np.float32), want)


@pytest.mark.parametrize("op", [0, 5])
def test_grid_stride_second_pass(L, op):
    """4096 workgroups of 256 threads is the cap: 4096 * 256 + 77 elements need a second pass of the grid-stride loop"""
    n = 4096 * 256 + 77
    rng = np.random.default_rng(42)
    s = rng.normal(size=(1, 1, 1, n)).astype(np.float32)
    s2 = rng.normal(size=(1, 1, 1, n)).astype(np.float32)
    g = Guarded(ro=("s", "s2"), s=s, s2=s2, d=(1, 1, 1, n))
    gop(L, op, g, ("d", 0), ("s", 0), ("s2", 0), 1, 1, 1, n, 0.5)
    want = np.float32(0.5) * s if op == 0 else np.where((s >= 0) & (s <= 1), s2, np.float32(0.0))
    assert np.array_equal(g.np("d").view(np.uint32), want.astype(np.float32).view(np.uint32))
