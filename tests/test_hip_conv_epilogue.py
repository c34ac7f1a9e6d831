"""The RRDB conv kernels one by one (conv3x3_mfma / conv3x3_s3x / conv3x3_h2x) through xsd_test_conv3x3_ex: the fused epilogue
of every kind the plans launch, the compact LeakyReLU' masks, the pixel-shuffled views on either side, the launchers' refusals and
the f16x3 max-|x| slots.

Reference: the formula of the OutDesc comment (csrc/xsd_kernels.h) over torch.nn.functional.conv2d, all in float64 on the CPU.
Bar: max|got - ref| <= 2e-5 * max|ref| per output plane, the single-layer bar of test_hip_kernels.py (a planted spike is left out of
the max|ref| that sets the bar, not out of the comparison).  Every output is pre-filled with NaN and must come back finite; every
plane a launch reads or writes lies between NaN guard bands and every plane it only reads must come back unchanged.
The slot tests (f16x3) compare float bits: a slot is a maximum of stored values, not an approximation of one."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util_hip import guarded_planes

pytestmark = pytest.mark.gpu

TOL = 2e-5
ACC, E1, E2, E3, MASK = 1, 2, 4, 8, 16                 # bits of an epilogue kind (csrc/conv3x3_h2x.hip)
OPERANDS = (("e1", E1), ("e2", E2), ("e3", E3), ("mask", MASK))
# distinct, non-trivial scalars: a swap of any two of them changes the result far above the bar
DISTINCT = dict(a1=0.2, s1=0.75, a2=0.3, s2=-1.25, s3=0.5, slope=0.2, mslope=0.01)
ENGINE_VALUES = dict(a1=0.2, s1=1.0, a2=0.2, s2=1.0)   # what the plan gives a dense block's / a residual block's last conv
BITS_GUARD = 8192                                       # 16-bit words in front of and behind a compact-mask buffer


def _engine(math):
    from xmm_superres_denoise.engine import Engine
    e = Engine("dn", 1, 1, 32, 1)
    e.set_math(math)
    assert e.get_math() == math
    return e


@pytest.fixture(scope="module", params=["fp32", "bf16x6", "f16x3"])
def eng(request):
    return _engine(request.param)


@pytest.fixture(scope="module", params=["bf16x6", "f16x3"])
def eng_split(request):
    return _engine(request.param)


@pytest.fixture(scope="module")
def eng_h2x():
    return _engine("f16x3")


def chunk(kind=0, **kw):
    """One output chunk: its kind bits, its scalars (the engine's neutral 1.0 unless given) and, optionally, its planes' contents
    (`e1_data`, `e2_data`, `e3_data`, `mask_data`, `dst_data`: [B, 32, H, W] float32), `bits_out` (bool) and `bits_in` (int16 tensor)."""
    d = dict(kind=kind, a1=1.0, s1=1.0, a2=1.0, s2=1.0, s3=1.0, slope=1.0, mslope=1.0, bits_out=False, bits_in=None)
    d.update(kw)
    return d


def to_plane(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()


def from_plane(t):
    return t.cpu().numpy().transpose(0, 3, 1, 2)


def unshuffle(hr):
    """[B, 32, 2H, 2W] -> [B, 128, H, W]: channel 32 n + c = sub-pixel view n = 2i + j of channel c (Builder::shuf_in)"""
    B, C, H2, W2 = hr.shape
    return hr.reshape(B, C, H2 // 2, 2, W2 // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 4 * C, H2 // 2, W2 // 2)


def make_inputs(rng, B, H, W, n_in, n_out, bias=True):
    x = rng.normal(size=(B, 32 * n_in, H, W)).astype(np.float32)
    w = (rng.normal(size=(32 * n_out, 32 * n_in, 3, 3)) / np.sqrt(288 * n_in)).astype(np.float32)
    b = rng.normal(size=(32 * n_out,)).astype(np.float32) if bias else None
    return x, w, b


def fill_operands(rng, chunks, B, H, W):
    """independent random planes for every operand a chunk's kind names and has no contents for yet"""
    for c in chunks:
        for name, bit in OPERANDS:
            if c["kind"] & bit and c.get(name + "_data") is None:
                c[name + "_data"] = rng.normal(size=(B, 32, H, W)).astype(np.float32)
        if c["kind"] & ACC and c.get("dst_data") is None:
            c["dst_data"] = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    return chunks


def reference(x, w, b, chunks, shuffle_in=False, shuffle_out=False):
    """float64: conv2d, then per chunk v = conv; v *= a1; (+= dst); (+= s1 e1); v *= a2; (+= s2 e2); (+= s3 e3); lrelu(slope); mask(mslope).
    The scalars are the float32 values the kernel is handed."""
    f32 = lambda v: float(np.float32(v))
    xt = torch.from_numpy(x).double()
    if shuffle_in:
        xt = unshuffle(xt)
    y = F.conv2d(xt, torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(), padding=1)
    outs = []
    for j, c in enumerate(chunks):
        t = lambda name: torch.from_numpy(c[name]).double()
        v = y[:, 32 * j:32 * j + 32] * f32(c["a1"])
        if c["kind"] & ACC:
            v = v + t("dst_data")
        if c["kind"] & E1:
            v = v + f32(c["s1"]) * t("e1_data")
        v = v * f32(c["a2"])
        if c["kind"] & E2:
            v = v + f32(c["s2"]) * t("e2_data")
        if c["kind"] & E3:
            v = v + f32(c["s3"]) * t("e3_data")
        v = torch.where(v > 0, v, v * f32(c["slope"]))
        if c["kind"] & MASK:
            v = torch.where(t("mask_data") > 0, v, v * f32(c["mslope"]))
        outs.append(v)
    if shuffle_out:      # pixel_shuffle of the conv's output with its channels laid out [n][c] (chunk n = sub-pixel 2i + j)
        B, _, H, W = outs[0].shape
        ync = torch.stack(outs, dim=1)                                          # [B][n][c][H][W]
        return [F.pixel_shuffle(ync.transpose(1, 2).reshape(B, 128, H, W), 2).numpy()]
    return [o.numpy() for o in outs]


def launch(eng, x, w, b, chunks, shuffle_in=False, shuffle_out=False, expect_rc=0):
    """One xsd_test_conv3x3_ex launch over guarded planes.  Returns (planes, amax, words): the output planes as [B, 32, H, W] numpy (one
    high-resolution plane with shuffle_out), the eleven max-|x| slots, and per chunk its compact-mask words [B, H, W, 2] uint16 or None."""
    from xmm_superres_denoise.engine._lib import XsdTestOut
    B = x.shape[0]
    H, W = (x.shape[2] // 2, x.shape[3] // 2) if shuffle_in else (x.shape[2], x.shape[3])
    n_in, n_out = (4 if shuffle_in else x.shape[1] // 32), len(chunks)
    assert w.shape == (32 * n_out, 32 * n_in, 3, 3)
    if shuffle_in:
        x_orig = [to_plane(x)]
        xin, chk_in = guarded_planes(1, B, 2 * H, 2 * W, x_orig)
    else:
        x_orig = [to_plane(x[:, 32 * i:32 * i + 32]) for i in range(n_in)]
        xin, chk_in = guarded_planes(n_in, B, H, W, x_orig)
    op_orig, op_slot = [], {}
    for j, c in enumerate(chunks):
        for name, bit in OPERANDS:
            if c["kind"] & bit:
                op_slot[(j, name)] = len(op_orig)
                op_orig.append(to_plane(c[name + "_data"]))
    ops, chk_ops = guarded_planes(len(op_orig), B, H, W, op_orig) if op_orig else ([], lambda: None)
    nan_plane = torch.full((B, H, W, 32), float("nan"), device="cuda")
    if shuffle_out:
        assert not any(c["kind"] & ACC for c in chunks)
        outs, chk_out = guarded_planes(1, B, 2 * H, 2 * W, None)
    else:
        outs, chk_out = guarded_planes(n_out, B, H, W, [to_plane(c["dst_data"]) if c["kind"] & ACC else nan_plane for c in chunks])
    before = [o.clone() for o in outs]
    nwords = B * H * W * 2
    words = [torch.full((2 * BITS_GUARD + nwords,), -1, dtype=torch.int16, device="cuda") if c["bits_out"] else None for c in chunks]
    bits_in_before = [c["bits_in"].clone() if c["bits_in"] is not None else None for c in chunks]
    descs = (XsdTestOut * n_out)()
    for j, c in enumerate(chunks):
        d = descs[j]
        d.p = outs[0 if shuffle_out else j].data_ptr()
        for name, _ in OPERANDS:
            setattr(d, name, ops[op_slot[(j, name)]].data_ptr() if (j, name) in op_slot else None)
        for name in ("a1", "s1", "a2", "s2", "s3", "slope", "mslope"):
            setattr(d, name, c[name])
        d.accumulate = 1 if c["kind"] & ACC else 0
        d.bits_out = words[j][BITS_GUARD:].data_ptr() if c["bits_out"] else None
        d.bits_in = c["bits_in"].data_ptr() if c["bits_in"] is not None else None
    in_ptrs = (ctypes.c_void_p * len(xin))(*[t.data_ptr() for t in xin])
    wd = torch.from_numpy(w).cuda()
    bd = torch.from_numpy(b).cuda() if b is not None else None
    amax = (ctypes.c_float * 11)(*([-1.0] * 11))
    rc = eng.L.xsd_test_conv3x3_ex(eng.h, in_ptrs, n_in, int(shuffle_in), wd.data_ptr(), bd.data_ptr() if bd is not None else None,
                                   descs, n_out, int(shuffle_out), amax, B, H, W, None)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, eng.L.xsd_last_error().decode())
    for c in (chk_in, chk_ops, chk_out):
        c()
    for a, o in zip(xin, x_orig):
        assert torch.equal(a, o), "an input plane was modified"
    for a, o in zip(ops, op_orig):
        assert torch.equal(a, o), "an operand plane was modified"
    assert torch.equal(wd, torch.from_numpy(w).cuda()) and (bd is None or torch.equal(bd, torch.from_numpy(b).cuda()))
    for c, o in zip(chunks, bits_in_before):
        assert o is None or torch.equal(c["bits_in"], o)
    for wj in words:      # no 16-bit word outside [B * H * W * 2] may change
        assert wj is None or (bool((wj[:BITS_GUARD] == -1).all()) and bool((wj[BITS_GUARD + nwords:] == -1).all())), "a mask word outside the image was written"
    if rc != 0:           # a refused launch writes nothing
        for o, o0 in zip(outs, before):
            assert torch.equal(torch.isnan(o), torch.isnan(o0)) and torch.equal(torch.nan_to_num(o), torch.nan_to_num(o0)), "a refused launch wrote its output"
        for wj in words:
            assert wj is None or bool((wj == -1).all()), "a refused launch wrote mask words"
        return None, None, None
    planes = [from_plane(o) for o in outs]
    for p in planes:
        assert np.isfinite(p).all(), "an output element was not written"
    wout = [wj[BITS_GUARD:BITS_GUARD + nwords].cpu().numpy().view(np.uint16).reshape(B, H, W, 2) if wj is not None else None for wj in words]
    return planes, np.array(list(amax), dtype=np.float32), wout


def assert_close(got, ref, what="", spike=None):
    """per output plane: max|got - ref| <= 2e-5 max|ref|; `spike` = (plane, b, c, y, x) is left out of max|ref| only"""
    for j, (g, r) in enumerate(zip(got, ref)):
        a = np.abs(r)
        if spike is not None and spike[0] == j:
            a = a.copy()
            a[spike[1:]] = 0.0
        err, bar = float(np.abs(g - r).max()), TOL * float(a.max())
        print(f"{what} plane {j}: max|got - ref| {err:.3e}  bar {bar:.3e}  ({err / (a.max() + 1e-300):.2e} of max|ref|)")
        assert err <= bar, f"{what} plane {j}: {err:.3e} > {bar:.3e}"


def run_case(eng, B, H, W, n_in, chunks, seed, what=""):
    rng = np.random.default_rng(seed)
    x, w, b = make_inputs(rng, B, H, W, n_in, len(chunks))
    fill_operands(rng, chunks, B, H, W)
    got, amax, _ = launch(eng, x, w, b, chunks)
    assert_close(got, reference(x, w, b, chunks), what)
    return got, amax


def pack_words(pos):
    """[B, 32, H, W] bool -> [B, H, W, 2] uint16: bit 4q + t of word [pixel][h] <-> channel 8q + 4h + t (OutDesc::bits_out)"""
    B, _, H, W = pos.shape
    p = pos.transpose(0, 2, 3, 1).reshape(B, H, W, 4, 2, 4).astype(np.uint32)          # [q][h][t]
    weight = (1 << (4 * np.arange(4)[:, None] + np.arange(4)[None, :])).astype(np.uint32)   # [q][t]
    return (p * weight[None, None, None, :, None, :]).sum(axis=(3, 5)).astype(np.uint16)


def bits_of(v):
    return int(np.float32(v).view(np.uint32))


# ---- every kind on its own ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_in", [1, 3])
@pytest.mark.parametrize("shape", [(2, 19, 45), (1, 8, 32)])
@pytest.mark.parametrize("kind", [0, E1, E1 | E2, E1 | E2 | E3, MASK, ACC, ACC | E1, ACC | E1 | E2])
def test_each_kind(eng, kind, shape, n_in):
    """kinds 0, 2, 6, 14, 16, and the accumulating 1, 3, 7 (the wide nets' final partial sum), each with the seven distinct scalars"""
    B, H, W = shape
    run_case(eng, B, H, W, n_in, [chunk(kind, **DISTINCT)], 1000 + 10 * kind + n_in, f"kind {kind}")


@pytest.mark.parametrize("n_in", [1, 3])
def test_kind_6_with_the_engines_values(eng, n_in):
    run_case(eng, 2, 19, 45, n_in, [chunk(E1 | E2, **ENGINE_VALUES)], 77 + n_in, "kind 6, engine values")


def test_mask_decision_at_zero(eng):
    """mask > 0 passes, everything else takes mslope: +0.0, -0.0 and -tiny scale by mslope, the smallest positive subnormal passes.
    Each of the four values fills whole image columns (every channel, every row), so the decision shows at thousands of entries."""
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(5)
    mask = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    specials = [np.float32(0.0), np.float32(-0.0), np.float32(1e-45), -np.finfo(np.float32).tiny]
    assert specials[2] > 0 and bits_of(specials[2]) == 1 and bits_of(specials[1]) == 0x80000000
    for k, v in enumerate(specials):
        mask[:, :, :, [3 + k, 31 + k, 40 + k]] = v
    c = chunk(MASK, mask_data=mask, **DISTINCT)
    x, w, b = make_inputs(rng, B, H, W, 1, 1)
    got, _, _ = launch(eng, x, w, b, [c])
    ref = reference(x, w, b, [c])
    assert_close(got, ref, "mask at zero")
    # and the decision itself, entry by entry: the two branches differ by a factor of 100, an entry on the wrong one is off by 99 % of itself
    for k in range(4):
        cols = [3 + k, 31 + k, 40 + k]
        g, r = got[0][:, :, :, cols], ref[0][:, :, :, cols]
        assert np.abs(g - r).max() <= 1e-3 * np.abs(r).max()
        big = np.abs(r) > 0.05 * np.abs(r).max()
        assert big.sum() > 100 and (np.abs(g - r)[big] <= 0.01 * np.abs(r)[big]).all(), f"mask value {specials[k]!r} took the wrong branch"


# ---- one epilogue, two code paths: an instance of its own and the catch-all kernel --------------------------------------------------

@pytest.mark.parametrize("kinds,slope", [
    ((E1, E1), 1.0),            # uniform kind 2 without a LeakyReLU: the kind's own instance where there is one
    ((E1, E1), 0.2),            # uniform kind 2 WITH a LeakyReLU: the instance has none, the launcher must fall back
    ((E1, 0), 1.0), ((E1, 0), 0.2),              # chunks of different kinds: the catch-all kernel
    ((MASK, E1), 1.0), ((MASK, E1), 0.2),
    ((MASK, MASK), 1.0), ((0, 0), 0.2),
])
def test_instance_and_catch_all_paths(eng, kinds, slope):
    sc = dict(DISTINCT, slope=slope)
    run_case(eng, 2, 19, 45, 1, [chunk(k, **sc) for k in kinds], 300 + kinds[0] + 7 * kinds[1], f"kinds {kinds} slope {slope}")


@pytest.mark.parametrize("n_out", [2, 4, 5])
def test_multi_output_with_per_chunk_epilogues(eng, n_out):
    kinds = [E1, 0, E1 | E2, MASK, E1 | E2 | E3][:n_out]
    chunks = [chunk(k, **{n: v * (1.0 + 0.25 * j) for n, v in DISTINCT.items() if n not in ("slope", "mslope")},
                    slope=[0.2, 0.01, 1.0, 0.5, 0.2][j], mslope=[0.01, 0.2, 0.5, 0.01, 0.3][j]) for j, k in enumerate(kinds)]
    run_case(eng, 2, 19, 45, 1, chunks, 400 + n_out, f"n_out {n_out}")


# ---- compact LeakyReLU' masks (split modes) --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 19, 45), (3, 5, 7)])
def test_compact_masks_written_and_read(eng_split, shape):
    """kind 64: a forward conv with slope 0.2 writes one 16-bit word per pixel and lane half; unpacked with the documented layout the
    words must equal `stored plane > 0` bit for bit (a chunk with zero weights and bias stores exactly 0: all bits clear).
    kind 48: the input-gradient conv masked by those words (and, kind 16, by the plane itself) against the float64 reference."""
    B, H, W = shape
    rng = np.random.default_rng(600 + H)
    x, w, b = make_inputs(rng, B, H, W, 1, 2)
    w[32:] = 0.0
    b[32:] = 0.0
    fwd = [chunk(0, slope=0.2, bits_out=True), chunk(0, slope=0.2, bits_out=True)]
    act, _, words = launch(eng_split, x, w, b, fwd)
    assert_close(act, reference(x, w, b, fwd), "kind 64")
    assert not act[1].any(), "zero weights and bias must store exactly 0"
    for j in range(2):
        assert np.array_equal(words[j], pack_words(act[j] > 0)), f"chunk {j}: compact mask != (stored plane > 0)"
    assert not words[1].any() and words[0].any()
    # backward: G -> dX masked by the activation of chunk 0, once through its words (kind 48) and once through the plane (kind 16)
    g, wt, _ = make_inputs(rng, B, H, W, 1, 1, bias=False)
    wdev = torch.from_numpy(words[0].view(np.int16).reshape(-1).copy()).cuda()
    res = {}
    for name, bits in (("kind 48", wdev), ("kind 16", None)):
        c = chunk(MASK, mask_data=act[0], mslope=0.2, bits_in=bits)
        res[name], _, _ = launch(eng_split, g, wt, None, [c])
        assert_close(res[name], reference(g, wt, None, [c]), name)
    print(f"kind 48 vs kind 16 on the same data: max difference {np.abs(res['kind 48'][0] - res['kind 16'][0]).max():.3e}")


# ---- pixel-shuffled views ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 19, 22)])
def test_shuffle_out(eng, shape):
    """1 input plane -> 4 chunks that interleave into ONE plane [B][2H][2W][32] (the SR head's upsampling conv, LeakyReLU 0.01)"""
    B, H, W = shape
    rng = np.random.default_rng(700 + H)
    x, w, b = make_inputs(rng, B, H, W, 1, 4)
    chunks = [chunk(0, slope=0.01) for _ in range(4)]
    got, amax, _ = launch(eng, x, w, b, chunks, shuffle_out=True)
    assert got[0].shape == (B, 32, 2 * H, 2 * W)
    assert_close(got, reference(x, w, b, chunks, shuffle_out=True), "shuffle_out")
    if eng.get_math() == "f16x3":      # ONE maximum per launch in all four views' slots: the high-resolution plane's
        views = unshuffle(torch.from_numpy(got[0])).numpy().reshape(B, 4, 32, H, W)
        for n in range(4):
            assert bits_of(amax[6 + n]) == bits_of(np.abs(got[0]).max()) and amax[6 + n] >= np.abs(views[:, n]).max()


@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 19, 22)])
def test_shuffle_in(eng, shape):
    """the four sub-pixel views of one high-resolution plane as K-steps -> 1 standard plane, masked (kind 16) as the backward plan does"""
    B, H, W = shape
    rng = np.random.default_rng(800 + H)
    xhr = rng.normal(size=(B, 32, 2 * H, 2 * W)).astype(np.float32)
    peaks = []
    for n in range(4):      # a distinct maximum in every view
        yy, xx, cc = 2 * (n + 1) + (n >> 1), 2 * (5 - n) + (n & 1), 7 * n + 3
        xhr[B - 1, cc, yy, xx] = -(6.0 + n)
        peaks.append(6.0 + n)
    w = (rng.normal(size=(32, 128, 3, 3)) / np.sqrt(288 * 4)).astype(np.float32)
    c = fill_operands(rng, [chunk(MASK, mslope=0.01)], B, H, W)
    got, amax, _ = launch(eng, xhr, w, None, c, shuffle_in=True)
    assert_close(got, reference(xhr, w, None, c, shuffle_in=True), "shuffle_in")
    if eng.get_math() == "f16x3":
        views = unshuffle(torch.from_numpy(xhr)).numpy().reshape(B, 4, 32, H, W)
        for n in range(4):
            assert np.abs(views[:, n]).max() == peaks[n]
            assert bits_of(amax[n]) == bits_of(peaks[n]), f"input slot {n}: {amax[n]} != {peaks[n]}"
        assert bits_of(amax[5]) == bits_of(np.abs(w).max()) and bits_of(amax[6]) == bits_of(np.abs(got[0]).max())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [E1, ACC])
def test_bits_out_with_an_operand_is_refused(eng_split, kind):
    """no epilogue variant writes compact masks next to an operand: the launcher says so (XSD_ERR_HIP) and nothing is written"""
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(900 + kind)
    x, w, b = make_inputs(rng, B, H, W, 1, 1)
    c = fill_operands(rng, [chunk(kind, slope=0.2, bits_out=True)], B, H, W)
    c[0]["dst_data"] = np.full((B, 32, H, W), np.nan, np.float32)       # (accumulate: the destination stays what it was, NaN)
    launch(eng_split, x, w, b, c, expect_rc=-2)
    # the engine stays usable
    run_case(eng_split, B, H, W, 1, [chunk(0, slope=0.2)], 901, "after a refusal")


# ---- more tiles than workgroups ---------------------------------------------------------------------------------------------------

BIG = (3, 100, 420)      # 294 tiles of 16 x 32 on a 256-CU grid, 546 of 8 x 32 on the fp32 kernel's 512: every workgroup walks several, ragged


@pytest.fixture(scope="module")
def big_case():
    """inputs and the float64 conv of the (3, 100, 420) case, computed once and left unchanged"""
    B, H, W = BIG
    rng = np.random.default_rng(4242)
    x, w, b = make_inputs(rng, B, H, W, 1, 1)
    e1 = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    y = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)
    return x, w, b, e1, y


def _big_ref(y, c):
    f32 = lambda v: float(np.float32(v))
    v = (y * f32(c["a1"]) + f32(c["s1"]) * torch.from_numpy(c["e1_data"]).double()) * f32(c["a2"])
    return [torch.where(v > 0, v, v * f32(c["slope"])).numpy()]


@pytest.mark.parametrize("slope", [1.0, 0.2])
def test_more_tiles_than_workgroups(eng, big_case, slope):
    """kind 2 at (3, 100, 420): without a LeakyReLU (f16x3: the kind's own instance) and with one (the catch-all kernel)"""
    x, w, b, e1, y = big_case
    c = chunk(E1, e1_data=e1, **dict(DISTINCT, slope=slope))
    got, _, _ = launch(eng, x, w, b, [c])
    assert_close(got, _big_ref(y, c), f"big, slope {slope}")


# ---- f16x3: the max-|x| slots -----------------------------------------------------------------------------------------------------

def _slot_case(eng_h2x, x, w, b, chunks, spike, ref=None):
    """the launch's slot (every chunk's: one maximum per launch) == max |stored values| over all chunks, as float bits; the input and
    weight slots == max |x| of what went in"""
    got, amax, _ = launch(eng_h2x, x, w, b, chunks)
    assert_close(got, reference(x, w, b, chunks) if ref is None else ref, "slot case", spike)
    stored = max(float(np.abs(g).max()) for g in got)
    j, bb, cc, yy, xx = spike
    assert abs(got[j][bb, cc, yy, xx]) == stored and stored > 900.0      # the planted entry IS the maximum
    for k in range(len(chunks)):
        assert bits_of(amax[6 + k]) == bits_of(stored), f"output slot {k}: {amax[6 + k]!r} != max|stored| {stored!r}"
    for i in range(x.shape[1] // 32):
        assert bits_of(amax[i]) == bits_of(np.abs(x[:, 32 * i:32 * i + 32]).max())
    assert bits_of(amax[5]) == bits_of(np.abs(w).max())


# (b, y, x, channel, chunk, n_out) at (2, 19, 45), 16 x 32 tiles: rows 0, 1, 14, 15 of a tile = the first and the last MFMA wave; tile columns
# 0 and 31; channels 0, 3, 4, 28, 31 = both lane halves, first and last quad; the last pixel of the ragged image; the last image; chunk 2 of 2
SPIKES = [
    (0, 0, 5, 0, 0, 1), (0, 1, 5, 3, 0, 1), (0, 14, 5, 4, 0, 1), (0, 15, 5, 28, 0, 1),
    (0, 7, 0, 31, 0, 1), (0, 7, 31, 0, 0, 1), (0, 7, 32, 4, 0, 1), (0, 16, 44, 28, 0, 1),
    (0, 18, 44, 31, 0, 1), (1, 18, 44, 0, 0, 1), (1, 3, 40, 28, 0, 1), (1, 9, 20, 3, 1, 2), (0, 15, 31, 31, 1, 2),
]


@pytest.mark.parametrize("b,y,x,c,j,n_out", SPIKES)
def test_slot_is_the_maximum_of_the_stored_values(eng_h2x, b, y, x, c, j, n_out):
    """the maximum is planted through e1 (s1 = 1, 1e3 at one entry): whichever lane, wave, tile and chunk holds it must publish it"""
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(1100 + 31 * y + x + c)
    xs, w, bias = make_inputs(rng, B, H, W, 1, n_out)
    chunks = fill_operands(rng, [chunk(E1) for _ in range(n_out)], B, H, W)
    chunks[j]["e1_data"][b, c, y, x] = 1e3
    _slot_case(eng_h2x, xs, w, bias, chunks, (j, b, c, y, x))


def test_slot_from_a_tile_that_is_not_its_workgroups_first(eng_h2x, big_case):
    """(3, 100, 420): 294 tiles on at most 256 workgroups, tile t runs as item t // G of workgroup t % G; the last tile (last image,
    bottom right) is never a workgroup's first"""
    x, w, b, e1, y = big_case
    B, H, W = BIG
    e1s = e1.copy()
    e1s[B - 1, 17, H - 1, W - 1] = 1e3
    c = chunk(E1, e1_data=e1s)
    _slot_case(eng_h2x, x, w, b, [c], (0, B - 1, 17, H - 1, W - 1), ref=_big_ref(y, c))


@pytest.mark.parametrize("edge", ["x = W", "y = H"])
def test_lanes_outside_the_image_do_not_count(eng_h2x, edge):
    """W = 45, H = 19: the tiles' lanes at x = 45 .. 63 and y = 19 .. 31 compute real sums from the halo.  With the one tap (ky 1, kx 0)
    out(y, x) = w in(y, x - 1): a 1e6 in input column W - 1 reaches NO output of the image, only the lane at x = W (and likewise
    tap (ky 0, kx 1) and input row H - 1 the lane at y = H).  The slot must still be the maximum of what was stored."""
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(1300 + len(edge))
    x = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    w = np.zeros((32, 32, 3, 3), np.float32)
    tap = rng.normal(size=(32, 32)).astype(np.float32) / np.float32(np.sqrt(32))
    if edge == "x = W":
        w[:, :, 1, 0] = tap
        x[:, :, :, W - 1] = 1e6
    else:
        w[:, :, 0, 1] = tap
        x[:, :, H - 1, :] = 1e6
    got, amax, _ = launch(eng_h2x, x, w, None, [chunk(0)])
    ref = reference(x, w, None, [chunk(0)])
    stored = float(np.abs(got[0]).max())
    # what the lanes outside hold is ~1e6 x the in-image values (their own conv sum): the case cannot pass by accident
    outside = float(np.abs(tap.astype(np.float64).sum(axis=1)).max()) * 1e6
    assert np.abs(ref[0]).max() < 100.0 and stored < 100.0 < 1e-3 * outside
    assert bits_of(amax[6]) == bits_of(stored), f"slot {amax[6]!r} != max|stored| {stored!r}: a lane outside the image was counted"
    assert bits_of(amax[0]) == bits_of(1e6) and bits_of(amax[5]) == bits_of(np.abs(w).max())
