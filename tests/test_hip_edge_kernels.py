"""The edge layers one by one (csrc/aux_kernels.hip: edge_expand 1 -> 32, edge_reduce 32 -> 1, edge_wgrad + edge_wgrad_final,
pack_edge) through xsd_test_edge_expand / xsd_test_edge_reduce / xsd_test_edge_wgrad: the engine's packer, launchers and block-count rule.

Reference: torch.nn.functional.conv2d plus the formula of the parameter structs (csrc/xsd_kernels.h), float64 on the CPU; the flipped
(input-gradient) forms and the weight gradients against autograd through conv2d.
Bars: outputs max|got - ref| <= 2e-5 max|ref| per tensor (a planted spike is left out of max|ref| only), dw / db 5e-5: the single-kernel
bars of test_hip_kernels.py for exact-fp32 kernels (here K = 9 or 288 fmaf terms).  Selects, clamps and max-|x| slots compare bits.
Every tensor of a launch lies between NaN guard bands in one allocation; outputs start as NaN; what a launch only reads must come back
bit for bit; what it does not own (other image channels, batch-stride gaps) keeps its NaN."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util_hip import Guarded

pytestmark = pytest.mark.gpu

TOL, TOL_DW = 2e-5, 5e-5
XSD_ERR_HIP = -2
BITS_GUARD = 8192
WORST = {}          # family -> worst measured error / max|ref| (printed per test; DESIGN.md section 21 quotes them)


@pytest.fixture(scope="module")
def eng():
    from xmm_superres_denoise.engine import Engine
    return Engine("dn", 1, 1, 32, 1)


def to_plane(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def from_plane(a):
    return a.transpose(0, 3, 1, 2)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def f32(v):
    return float(np.float32(v))


def bits_of(v):
    return int(np.float32(v).view(np.uint32))


def assert_close(got, ref, family, what="", tol=TOL, exclude=None):
    a = np.abs(ref)
    if exclude is not None:
        a = np.where(exclude, 0.0, a)
    scale = float(a.max())
    err = float(np.abs(got - ref).max())
    rel = err / (scale + 1e-300)
    WORST[family] = max(WORST.get(family, 0.0), rel)
    print(f"{family} {what}: max|got - ref| {err:.3e} = {rel:.2e} of max|ref| {scale:.3e} (worst so far {WORST[family]:.2e})")
    assert err <= tol * scale, f"{family} {what}: {err:.3e} > {tol * scale:.3e}"


def make_w_first(rng, cin):
    return (rng.normal(size=(32, cin, 3, 3)) / 3.0).astype(np.float32)


def make_w_last(rng, cout):
    return (rng.normal(size=(cout, 32, 3, 3)) / np.sqrt(288.0)).astype(np.float32)


def wblock(wfull, w_last, idx):
    """the (32, 9) block a hook packs: W_last[idx] or W_first[:, idx]"""
    return (wfull[idx] if w_last else wfull[:, idx]).reshape(32, 9)


# =====================================================================================================================================
# edge_expand
# =====================================================================================================================================

def run_expand(eng, img, ch, wfull, w_last=0, idx=0, flipped=0, bias=None, out0=None, mask=None, mslope=1.0, bits=None, amax=False,
               expect_rc=0):
    """img [B, C, H, W]: channel `ch` is read (C > 1: s_bs = C H W).  out0 [B, 32, H, W]: accumulate onto it.  Returns (out [B, 32, H, W],
    slot bits or None), or None for a refused launch (checked to have written nothing)."""
    B, C, H, W = img.shape
    items = dict(img=img, w=wfull, out=to_plane(out0) if out0 is not None else (B, H, W, 32))
    if bias is not None:
        items["bias"] = bias
    if mask is not None:
        items["mask"] = to_plane(mask)
    if amax:
        items["amax"] = np.zeros(1, np.float32)
    g = Guarded(ro=[k for k in items if k not in ("out", "amax")], **items)
    words = None
    if bits is not None:
        n = bits.size
        words = torch.full((2 * BITS_GUARD + n,), -1, dtype=torch.int16, device="cuda")
        words[BITS_GUARD:BITS_GUARD + n] = torch.from_numpy(bits.view(np.int16).reshape(-1).copy()).cuda()
        words_before = words.clone()
    rc = eng.L.xsd_test_edge_expand(eng.h, g.ptr("img", ch * H * W), C * H * W if C > 1 else 0, g.ptr("w", idx * (288 if w_last else 9)),
                                    int(w_last), int(flipped), 9 * wfull.shape[1], g.ptr("bias"), g.ptr("out"), g.ptr("mask"), mslope,
                                    words[BITS_GUARD:].data_ptr() if words is not None else None, int(out0 is not None), g.ptr("amax"),
                                    B, H, W, None)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, eng.L.xsd_last_error().decode())
    g.check()
    assert words is None or torch.equal(words, words_before), "the compact mask words were modified"
    if rc != 0:
        g.check(untouched=[k for k in ("out", "amax") if k in g.t])
        return None
    out = from_plane(g.np("out"))
    assert np.isfinite(out).all(), "an output element was not written"
    return out, (int(g.np("amax").view(np.uint32)[0]) if amax else None)


def ref_expand(s, blk, flipped=0, bias=None, out0=None, pos=None, mslope=1.0):
    """float64.  s [B, H, W]; blk (32, 9); pos: boolean [B, 32, H, W], where the mask decides `keep`."""
    k = torch.from_numpy(blk).double().reshape(32, 1, 3, 3)
    if flipped:
        k = k.flip(2, 3)
    v = F.conv2d(torch.from_numpy(s).double()[:, None], k, None if bias is None else torch.from_numpy(bias).double(), padding=1).numpy()
    if out0 is not None:
        v = v + out0.astype(np.float64)
    if pos is not None:
        v = np.where(pos, v, v * f32(mslope))
    return v


EXPAND_SHAPES = [(1, 1, 1), (2, 19, 45), (1, 3, 31), (1, 3, 32), (1, 3, 33), (1, 3, 510), (1, 3, 511), (2, 400, 8)]


@pytest.mark.parametrize("form", ["plain", "bias", "s_bs", "accumulate", "mask", "mask_accumulate"])
@pytest.mark.parametrize("shape", EXPAND_SHAPES)
def test_expand_forms(eng, shape, form):
    """(1, 3, 510): 3 (W + 2) = 1536 = one staging round exactly; 511: the first width with a second round; (2, 400, 8): 800 rows on 768
    workgroups.  s_bs: channel 1 of a three-channel image whose other channels hold NaN, with W_first[:, 1] (first_cstride 27)."""
    B, H, W = shape
    rng = np.random.default_rng(seed_of(shape, form))
    C, ch = (3, 1) if form == "s_bs" else (1, 0)
    img = np.full((B, C, H, W), np.nan, np.float32)
    img[:, ch] = rng.normal(size=(B, H, W))
    wf = make_w_first(rng, C)
    bias = None if form == "plain" else rng.normal(size=32).astype(np.float32)
    out0 = rng.normal(size=(B, 32, H, W)).astype(np.float32) if "accumulate" in form else None
    mask = rng.normal(size=(B, 32, H, W)).astype(np.float32) if "mask" in form else None
    mslope = {"mask": 0.2, "mask_accumulate": 0.01}.get(form, 1.0)
    out, _ = run_expand(eng, img, ch, wf, idx=ch, bias=bias, out0=out0, mask=mask, mslope=mslope)
    ref = ref_expand(img[:, ch], wblock(wf, 0, ch), 0, bias, out0, None if mask is None else mask > 0, mslope)
    assert_close(out, ref, "edge_expand", f"{form} {shape}")


@pytest.mark.parametrize("accumulate", [0, 1])
def test_expand_mask_decision_at_zero(eng, accumulate):
    """mask > 0 keeps the value, everything else takes mslope: +0.0, -0.0 and -tiny scale, the smallest subnormal keeps.  Each special fills
    whole image columns.  Without accumulate the mask is the prefetched operand, with it the kernel reads the mask on its own."""
    B, H, W = 2, 5, 45
    rng = np.random.default_rng(50 + accumulate)
    img = rng.normal(size=(B, 1, H, W)).astype(np.float32)
    wf, bias = make_w_first(rng, 1), rng.normal(size=32).astype(np.float32)
    mask = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    specials = [np.float32(0.0), np.float32(-0.0), np.float32(1e-45), -np.finfo(np.float32).tiny]
    assert specials[2] > 0 and bits_of(specials[2]) == 1 and bits_of(specials[1]) == 0x80000000
    for k, v in enumerate(specials):
        mask[:, :, :, [1 + k, 31 + k, 40 + k]] = v
    out0 = rng.normal(size=(B, 32, H, W)).astype(np.float32) if accumulate else None
    out, _ = run_expand(eng, img, 0, wf, bias=bias, out0=out0, mask=mask, mslope=-3.0)
    ref = ref_expand(img[:, 0], wblock(wf, 0, 0), 0, bias, out0, mask > 0, -3.0)
    assert_close(out, ref, "edge_expand", f"mask at zero, accumulate {accumulate}")
    keep = ref_expand(img[:, 0], wblock(wf, 0, 0), 0, bias, out0)
    for k, want_keep in enumerate([False, False, True, False]):      # the decision itself, away from any tolerance: the sign of out / keep
        cols = [1 + k, 31 + k, 40 + k]
        big = np.abs(keep[..., cols]) > 1e-3
        assert (np.sign(out[..., cols])[big] == (1 if want_keep else -1) * np.sign(keep[..., cols])[big]).all(), f"special {k}"


def pack_words(pos):
    """[B, 32, H, W] bool -> [B, H, W, 2] uint16: bit 4q + t of word [pixel][h] <-> channel 8q + 4h + t (OutDesc::bits_out)"""
    B, _, H, W = pos.shape
    p = pos.transpose(0, 2, 3, 1).reshape(B, H, W, 4, 2, 4).astype(np.uint32)
    weight = (1 << (4 * np.arange(4)[:, None] + np.arange(4)[None, :])).astype(np.uint32)
    return (p * weight[None, None, None, :, None, :]).sum(axis=(3, 5)).astype(np.uint16)


@pytest.mark.parametrize("math", ["bf16x6", "f16x3"])
def test_expand_reads_the_words_a_conv_wrote(math):
    """Producer and consumer of the compact LeakyReLU' mask pinned to ONE mapping: a split-mode conv (xsd_test_conv3x3_ex, kind 64: slope 0.2,
    bits_out) stores a plane with a known sign pattern -- per pixel exactly one of the channels 0, 3, 4, 15, 16, 28, 31 positive in a third
    of the image, random signs in the rest -- and writes its words; edge_expand masked by those words must match the float64 reference masked
    by `stored > 0`."""
    from test_hip_conv_epilogue import _engine, chunk, launch
    e = _engine(math)
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(77)
    marks = [0, 3, 4, 15, 16, 28, 31]
    x = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    x[np.abs(x) < 0.05] = 0.5
    want = x > 0
    pix = np.arange(H * W).reshape(H, W)
    third = pix % 3 == 0
    for k, c in enumerate(marks):
        sel = third & ((pix // 3) % 7 == k)
        x[:, :, sel] = -np.abs(x[:, :, sel])
        x[:, c, sel] = 1.0 + k
    want = x > 0
    for k, c in enumerate(marks):
        sel = third & ((pix // 3) % 7 == k)
        assert sel.any() and want[:, c][:, sel].all() and want[:, :, sel].sum(axis=1).max() == 1
    w = np.zeros((32, 32, 3, 3), np.float32)
    w[np.arange(32), np.arange(32), 1, 1] = 1.0                       # the identity conv: stored = lrelu(x), the sign of x
    act, _, words = launch(e, x, w, None, [chunk(0, slope=0.2, bits_out=True)])
    stored = act[0]
    assert np.array_equal(stored > 0, want), "the producer did not store the planned sign pattern"
    assert np.array_equal(words[0], pack_words(stored > 0)), "the conv's words != (stored plane > 0) under the documented layout"
    dy = rng.normal(size=(B, 1, H, W)).astype(np.float32)
    wl = make_w_last(rng, 1)
    out, _ = run_expand(e, dy, 0, wl, w_last=1, flipped=1, bits=words[0], mslope=0.2)
    ref = ref_expand(dy[:, 0], wblock(wl, 1, 0), 1, None, None, stored > 0, 0.2)
    assert_close(out, ref, "edge_expand", f"compact words of a {math} conv")


AMAX_CASES = [((2, 19, 45), (0, 0, 0)), ((2, 19, 45), (0, 7, 44)), ((2, 19, 45), (1, 18, 44)), ((2, 400, 8), (1, 390, 5)), ((1, 3, 511), (0, 2, 510))]


@pytest.mark.parametrize("shape,at", AMAX_CASES)
def test_expand_amax_slot(eng, shape, at):
    """The slot holds max |out| of the STORED values as float bits, wherever the maximum lies: the first pixel, the last pixel of a ragged
    row (45 = 32 + 13), the last image, row 790 of 800 (not its workgroup's first), the last pixel of the second staging round."""
    B, H, W = shape
    rng = np.random.default_rng(300 + at[1])
    img = rng.normal(size=(B, 1, H, W)).astype(np.float32)
    img[(at[0], 0) + at[1:]] = 30.0
    wf, bias = make_w_first(rng, 1), rng.normal(size=32).astype(np.float32)
    out, slot = run_expand(eng, img, 0, wf, bias=bias, amax=True)
    ref = ref_expand(img[:, 0], wblock(wf, 0, 0), 0, bias)
    near = np.zeros((B, 1, H, W), bool)
    near[at[0], 0, max(at[1] - 1, 0):at[1] + 2, max(at[2] - 1, 0):at[2] + 2] = True
    assert_close(out, ref, "edge_expand", f"amax {shape} at {at}", exclude=np.broadcast_to(near, ref.shape))
    where = np.unravel_index(np.abs(out).argmax(), out.shape)
    assert near[where[0], 0, where[2], where[3]], "the planted spike does not hold the maximum"
    assert slot == bits_of(np.abs(out).max()), (hex(slot), hex(bits_of(np.abs(out).max())))


def test_expand_amax_with_accumulate_is_refused(eng):
    """the kernel would report partial sums of a plane other launches complete: refused before the launch, nothing written"""
    rng = np.random.default_rng(9)
    img = rng.normal(size=(2, 1, 5, 7)).astype(np.float32)
    out0 = rng.normal(size=(2, 32, 5, 7)).astype(np.float32)
    assert run_expand(eng, img, 0, make_w_first(rng, 1), out0=out0, amax=True, expect_rc=XSD_ERR_HIP) is None


@pytest.mark.parametrize("shape", [(2, 19, 45), (1, 3, 33)])
@pytest.mark.parametrize("cout,o", [(1, 0), (3, 2)])
def test_expand_backward_form_vs_autograd(eng, shape, cout, o):
    """dT of conv_last for output channel o: the flipped packed form of W_last[o] against autograd through conv2d"""
    B, H, W = shape
    rng = np.random.default_rng(400 + cout + H)
    wl = make_w_last(rng, cout)
    dy = np.full((B, cout, H, W), np.nan, np.float32)
    dy[:, o] = rng.normal(size=(B, H, W))
    out, _ = run_expand(eng, dy, o, wl, w_last=1, idx=o, flipped=1)
    T = torch.zeros(B, 32, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(T, torch.from_numpy(wl[o:o + 1]).double(), padding=1)
    dT, = torch.autograd.grad(y, T, torch.from_numpy(dy[:, o:o + 1]).double())
    assert_close(out, dT.numpy(), "edge_expand", f"dT {shape} W_last[{o}] of {cout}")


# =====================================================================================================================================
# edge_reduce
# =====================================================================================================================================

def run_reduce(eng, f, wfull, w_last=1, idx=0, flipped=0, bias=None, skip=None, skip_ch=0, ny=1, y_ch=0, pre=False, clamp01=0, addto=None,
               allow_nonfinite=False):
    """f [B, 32, H, W].  y (and pre, addto) are channel y_ch of [B, ny, H, W] tensors, skip channel skip_ch of [B, C, H, W].
    Returns (y [B, H, W], pre or None)."""
    B, _, H, W = f.shape
    items = dict(f=to_plane(f), w=wfull, y=(B, ny, H, W))
    if bias is not None:
        items["bias"] = np.asarray([bias], np.float32)
    if skip is not None:
        items["skip"] = skip
    if pre:
        items["pre"] = (B, ny, H, W)
    if addto is not None:
        items["addto"] = addto
    g = Guarded(ro=[k for k in items if k not in ("y", "pre")], **items)
    HW = H * W
    rc = eng.L.xsd_test_edge_reduce(eng.h, g.ptr("f"), g.ptr("w", idx * (288 if w_last else 9)), int(w_last), int(flipped), 9 * wfull.shape[1],
                                    g.ptr("bias"), g.ptr("skip", skip_ch * HW), (skip.shape[1] * HW if skip is not None and skip.shape[1] > 1 else 0),
                                    g.ptr("pre", y_ch * HW), g.ptr("y", y_ch * HW), ny * HW if ny > 1 else 0, int(clamp01),
                                    g.ptr("addto", y_ch * HW), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, eng.L.xsd_last_error().decode())
    g.check()
    res = []
    for name in ("y", "pre"):
        if name not in g.t:
            res.append(None)
            continue
        a = g.np(name)
        other = [c for c in range(ny) if c != y_ch]
        assert np.isnan(a[:, other]).all(), f"{name}: a channel the launch does not own was written"
        assert allow_nonfinite or np.isfinite(a[:, y_ch]).all(), f"{name}: an element was not written"
        res.append(a[:, y_ch])
    return res


def ref_reduce(f, blk, flipped=0, bias=None, skip=None, addto=None, clamp01=0):
    k = torch.from_numpy(blk).double().reshape(1, 32, 3, 3)
    if flipped:
        k = k.flip(2, 3)
    with np.errstate(invalid="ignore"):
        v = F.conv2d(torch.from_numpy(f).double(), k, None if bias is None else torch.tensor([f32(bias)], dtype=torch.float64), padding=1)[:, 0]
        if skip is not None:
            v = v + torch.from_numpy(skip).double()
        if addto is not None:
            v = v + torch.from_numpy(addto).double()
    return (v.clamp(0, 1) if clamp01 else v).numpy(), v.numpy()


REDUCE_SHAPES = [(1, 1, 1), (2, 19, 45), (1, 33, 33), (1, 64, 32), (1, 65, 31), (8193, 1, 1)]


@pytest.mark.parametrize("form", ["plain", "bias", "skip_bs", "y_bs_pre_addto", "addto", "pre_clamp"])
@pytest.mark.parametrize("shape", REDUCE_SHAPES)
def test_reduce_forms(eng, shape, form):
    """ragged against the 32-column strip and the 32-row band on both sides; (8193, 1, 1): more blocks than the 8192-workgroup cap.
    skip_bs / y_bs: channel 1 of three-channel tensors whose other channels hold NaN (read side) or must keep it (write side)."""
    B, H, W = shape
    rng = np.random.default_rng(seed_of(shape, form))
    f = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    wl = make_w_last(rng, 2)
    kw, rkw = {}, {}
    if form != "plain":
        kw["bias"] = rkw["bias"] = 0.3
    if form == "skip_bs":
        skip = np.full((B, 3, H, W), np.nan, np.float32)
        skip[:, 1] = rng.uniform(size=(B, H, W))
        kw.update(skip=skip, skip_ch=1)
        rkw["skip"] = skip[:, 1]
    if form in ("y_bs_pre_addto", "addto"):
        ny, ch = (3, 1) if form == "y_bs_pre_addto" else (1, 0)
        addto = np.full((B, ny, H, W), np.nan, np.float32)
        addto[:, ch] = rng.normal(size=(B, H, W))
        kw.update(addto=addto, ny=ny, y_ch=ch, pre=form == "y_bs_pre_addto")
        rkw["addto"] = addto[:, ch]
    if form == "pre_clamp":
        skip = rng.uniform(size=(B, 1, H, W)).astype(np.float32)
        kw.update(skip=skip, pre=True, clamp01=1)
        rkw.update(skip=skip[:, 0], clamp01=1)
    y, pre = run_reduce(eng, f, wl, idx=1, **kw)
    ref_y, ref_pre = ref_reduce(f, wblock(wl, 1, 1), **rkw)
    if pre is not None:
        assert_close(pre, ref_pre, "edge_reduce", f"{form} {shape} pre")
        want = np.clip(pre, 0.0, 1.0) if kw.get("clamp01") else pre
        assert np.array_equal(y, want), "y is not the clamp of the pre-clamp value the kernel returned"
        if kw.get("clamp01") and B * H * W > 100:
            assert (pre < 0).any() and (pre > 1).any(), "the case does not reach both bounds"
    else:
        assert_close(y, ref_y, "edge_reduce", f"{form} {shape}")


def test_reduce_clamp_at_the_bounds(eng):
    """Zero weights and bias: the value is the skip operand exactly.  0, 1 and -0.0 stay, +-inf go to the bounds, NaN propagates (torch.clamp),
    values next to the bounds clamp; pre returns the operand itself."""
    B, H, W = 1, 3, 40
    tiny = np.finfo(np.float32).tiny
    specials = np.array([0.0, 1.0, -0.0, np.inf, -np.inf, np.nan, -tiny, np.nextafter(np.float32(1), np.float32(2)), 0.5, 1e-45], np.float32)
    skip = np.full((B, 1, H, W), 0.25, np.float32)
    skip[0, 0, 1, 5:5 + len(specials)] = specials
    skip[0, 0, 2, 39] = np.nan
    f = np.random.default_rng(3).normal(size=(B, 32, H, W)).astype(np.float32)
    y, pre = run_reduce(eng, f, np.zeros((1, 32, 3, 3), np.float32), bias=0.0, skip=skip, pre=True, clamp01=1, allow_nonfinite=True)
    want_pre = (np.float32(0.0) + skip[:, 0]).astype(np.float32)
    assert np.array_equal(pre.view(np.uint32), want_pre.view(np.uint32)), "pre is not the operand bit for bit"
    with np.errstate(invalid="ignore"):
        want = torch.from_numpy(want_pre).clamp(0, 1).numpy()
    assert np.array_equal(np.isnan(y), np.isnan(want)) and np.isnan(y).sum() == 2
    assert np.array_equal(np.nan_to_num(y, nan=7.0), np.nan_to_num(want, nan=7.0))
    assert y[0, 1, 5 + 3] == 1.0 and y[0, 1, 5 + 4] == 0.0 and y[0, 1, 5 + 6] == 0.0 and y[0, 1, 5 + 7] == 1.0


def test_reduce_nan_reaches_its_support_only(eng):
    """a NaN in one feature element: exactly the 3 x 3 pixels whose support holds it are NaN (in y through the clamp too), the rest is within the bar"""
    B, H, W = 2, 19, 45
    rng = np.random.default_rng(4)
    f = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    f[1, 17, 9, 31] = np.nan
    wl = make_w_last(rng, 1)
    y, pre = run_reduce(eng, f, wl, bias=0.3, pre=True, clamp01=1, allow_nonfinite=True)
    support = np.zeros((B, H, W), bool)
    support[1, 8:11, 30:33] = True
    assert np.array_equal(np.isnan(pre), support) and np.array_equal(np.isnan(y), support)
    ref_y, ref_pre = ref_reduce(np.nan_to_num(f), wblock(wl, 1, 0), bias=0.3, clamp01=1)
    assert_close(np.where(support, 0, pre), np.where(support, 0, ref_pre), "edge_reduce", "NaN support")
    assert np.array_equal(y[~support], np.clip(pre[~support], 0, 1))


@pytest.mark.parametrize("shape", [(2, 19, 45), (1, 33, 33)])
def test_reduce_poisoned_first_pixel(eng, shape):
    """Out-of-image taps READ the image's first pixel and select zero.  With inf there every output outside rows 0-1 x columns 0-1 must be
    finite and within the bar (a product with zero instead of the select makes every border pixel NaN)."""
    B, H, W = shape
    rng = np.random.default_rng(5)
    f = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    f[:, :, 0, 0] = np.inf
    wl = make_w_last(rng, 1)
    y, _ = run_reduce(eng, f, wl, bias=0.3, allow_nonfinite=True)
    clean = f.copy()
    clean[:, :, 0, 0] = 0.0
    ref, _ = ref_reduce(clean, wblock(wl, 1, 0), bias=0.3)
    near = np.zeros((B, H, W), bool)
    near[:, :2, :2] = True
    assert np.isfinite(y[~near]).all(), "the poisoned first pixel leaked into a pixel that does not see it"
    assert_close(np.where(near, 0, y), np.where(near, 0, ref), "edge_reduce", f"poisoned first pixel {shape}")
    assert not np.isfinite(y[near]).any()


@pytest.mark.parametrize("shape", [(2, 19, 45), (1, 65, 31)])
@pytest.mark.parametrize("cin,ch,with_addto", [(1, 0, False), (3, 2, False), (3, 1, True)])
def test_reduce_backward_form_vs_autograd(eng, shape, cin, ch, with_addto):
    """dx of conv_first for image channel ch: the flipped packed form of W_first[:, ch] (first_cstride 9 cin), written into channel ch of
    dx [B, cin, H, W]; with addto the DN skip gradient rides along (dx = dgrad + d out)."""
    B, H, W = shape
    rng = np.random.default_rng(600 + cin + ch + H)
    wf = make_w_first(rng, cin) * np.float32(0.2)
    dfea = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    addto = None
    if with_addto:
        addto = np.full((B, cin, H, W), np.nan, np.float32)
        addto[:, ch] = rng.normal(size=(B, H, W))
    y, _ = run_reduce(eng, dfea, wf, w_last=0, idx=ch, flipped=1, ny=cin, y_ch=ch, addto=addto)
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, requires_grad=True)
    dx, = torch.autograd.grad(F.conv2d(x, torch.from_numpy(wf).double(), padding=1), x, torch.from_numpy(dfea).double())
    ref = dx[:, ch].numpy() + (addto[:, ch].astype(np.float64) if with_addto else 0.0)
    assert_close(y, ref, "edge_reduce", f"dx {shape} channel {ch} of {cin}")


# =====================================================================================================================================
# edge_wgrad + edge_wgrad_final
# =====================================================================================================================================

def run_wgrad(eng, f, s, ch, mode, cin=1, nblocks=0):
    """f [B, 32, H, W]; s [B, C, H, W], channel ch.  mode 0: dw = channel ch of a NaN [32][cin][9] (cstride 9 cin), db [32]; mode 1: dw [32][9],
    db[0] of a NaN [32].  Returns (dw buffer, db buffer, nblocks that ran)."""
    B, C, H, W = s.shape
    g = Guarded(ro=("f", "s"), f=to_plane(f), s=s, dw=(32, cin if mode == 0 else 1, 9), db=(32,))
    used = ctypes.c_int(-1)
    rc = eng.L.xsd_test_edge_wgrad(eng.h, g.ptr("f"), g.ptr("s", ch * H * W), C * H * W if C > 1 else 0, mode, g.ptr("dw", ch * 9 if mode == 0 else 0),
                                   g.ptr("db"), 9 * cin if mode == 0 else 9, nblocks, ctypes.byref(used), B, H, W, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, eng.L.xsd_last_error().decode())
    g.check()
    return g.np("dw"), g.np("db"), used.value


def ref_wgrad(f, s1, mode):
    """autograd, float64.  mode 0: fea = conv2d(x, W[32, 1]), upstream f -> (dW [32, 9], db [32]); mode 1: y = conv2d(T = f, W[1, 32]) + b,
    upstream s -> (dW [32, 9], db [1])"""
    ft, st = torch.from_numpy(f).double(), torch.from_numpy(s1).double()[:, None]
    if mode == 0:
        w = torch.zeros(32, 1, 3, 3, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(32, dtype=torch.float64, requires_grad=True)
        dw, db = torch.autograd.grad(F.conv2d(st, w, b, padding=1), (w, b), ft)
        return dw.reshape(32, 9).numpy(), db.numpy()
    w = torch.zeros(1, 32, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    dw, db = torch.autograd.grad(F.conv2d(ft, w, b, padding=1), (w, b), st)
    return dw.reshape(32, 9).numpy(), db.numpy()


WGRAD_SHAPES = [(2, 19, 45), (3, 5, 7), (1, 2, 1), (1, 3, 96), (1, 3, 97), (1, 3, 128), (1, 3, 129)]


@pytest.mark.parametrize("nblocks", [1, 7, 0])
@pytest.mark.parametrize("mode,cin,ch", [(0, 1, 0), (0, 3, 1), (1, 3, 1)])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad(eng, shape, mode, cin, ch, nblocks):
    """Widths 96 / 97 / 128 / 129 lie on both sides of the four-deep sweep `x + 96 < W`.  nblocks 1, 7 (below and, for the small shapes,
    above the row count) and the engine's rule (2048 > B H: idle workgroups must contribute zeros).  cin 3: s is channel 1 of a three-channel
    image (s_bs != 0, NaN in the others); in mode 0 the launch writes channel 1 of dW [32][3][9] (cstride 27) and the others keep their NaN.
    s has mean 0.5 so that db[0] = sum s of mode 1 is a well-conditioned sum.  Two runs are bitwise equal."""
    B, H, W = shape
    rng = np.random.default_rng(seed_of(shape, mode, cin))
    f = rng.normal(size=(B, 32, H, W)).astype(np.float32)
    s = np.full((B, cin, H, W), np.nan, np.float32)
    s[:, ch] = rng.normal(size=(B, H, W)) + 0.5
    dw, db, used = run_wgrad(eng, f, s, ch, mode, cin, nblocks)
    assert used == (nblocks or 2048) and (nblocks or used > B * H)
    dw2, db2, _ = run_wgrad(eng, f, s, ch, mode, cin, nblocks)
    assert np.array_equal(dw.view(np.uint32), dw2.view(np.uint32)) and np.array_equal(db.view(np.uint32), db2.view(np.uint32)), "two runs differ"
    ref_dw, ref_db = ref_wgrad(f, s[:, ch], mode)
    if mode == 0:
        other = [c for c in range(cin) if c != ch]
        assert np.isnan(dw[:, other]).all(), "a channel of dW the launch does not own was written"
        assert_close(dw[:, ch], ref_dw, "edge_wgrad", f"mode 0 dw {shape} nblocks {used}", TOL_DW)
        assert_close(db, ref_db, "edge_wgrad", f"mode 0 db {shape} nblocks {used}", TOL_DW)
    else:
        assert_close(dw[:, 0], ref_dw, "edge_wgrad", f"mode 1 dw {shape} nblocks {used}", TOL_DW)
        assert np.isnan(db[1:]).all(), "mode 1 writes db[0] only"
        assert_close(db[:1], ref_db, "edge_wgrad", f"mode 1 db {shape} nblocks {used}", TOL_DW)


def test_wgrad_refuses_more_blocks_than_the_partial_buffer_holds(eng):
    f = np.zeros((1, 32, 2, 2), np.float32)
    g = Guarded(ro=("f", "s"), f=to_plane(f), s=np.zeros((1, 1, 2, 2), np.float32), dw=(32, 1, 9), db=(32,))
    rc = eng.L.xsd_test_edge_wgrad(eng.h, g.ptr("f"), g.ptr("s"), 0, 0, g.ptr("dw"), g.ptr("db"), 9, 2049, None, 1, 2, 2, None)
    assert rc == -1
    g.check(untouched=("dw", "db"))
