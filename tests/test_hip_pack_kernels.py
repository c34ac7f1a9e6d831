"""The weight-pack, fp16-split, width-padding and add_channels kernels one by one (csrc/aux_kernels.hip: pack_weights_kernel,
pack_weights_s3_kernel, buffer_amax_kernel, split_panels_f16_kernel, pack_edge_kernel, pack_shuffle_bias_kernel, add_channels_kernel;
csrc/xsd_engine.hip: pad_params_kernel), through the engine's own descriptor table and xsd_pack_weights.  What a pack left in device
memory is read back region by region (include/xsd.h: xsd_test_packed_region) and compared BIT FOR BIT, over the whole region, with numpy
written from the layout comments above the kernels:
  fp32 panels (mode fp32)        fwd [n][s][tap][j][h][co][t] = W[oc(n, co)][32 s + 16 h + 4 j + t][tap], panel n * ns + s
                                 bwd [s][n][tap'][j][h][ci][t] = bwd_scale * W[oc(n, 16 h + 4 j + t)][32 s + ci][8 - tap'], panel s * nn + n
  fragment panels (bf16x6, f16x3) [s2][tap][lane = 32 h + m][j], k = 16 s2 + 8 h + j; row m the output (dgrad: input) channel
  f16x3 image                    [panel][s2][tap][term h | l][lane][8 x f16] of split2(panel, scale_for_amax(slot)), tests/test_split_math.py
  pixel-shuffle convs            chunk n = sub-pixel * P + plane; the permutation is taken from torch's pixel_shuffle, not from the kernel.
Two fills of the flat parameter vector: index codes (element i holds float(i + 1), exact below 2^24, so every packed float names the
parameter it came from) and seeded random weights (randn / sqrt(9 cin))."""
import ctypes

import numpy as np
import pytest
import torch

from test_split_math import scale_for_amax, split2
from util_hip import Guarded

pytestmark = pytest.mark.gpu

PANEL = 9216      # csrc/xsd_kernels.h: PANEL_FLOATS
REGION = {"pk_fwd": 0, "pk_bwd": 1, "pk_fwd_s": 2, "pk_bwd_s": 3, "amax": 4, "pk_edge": 5, "pk_sbias": 6, "params_pad": 7, "table": 8}
ERR_ARG, ERR_STATE = -1, -3
MODES = {0: "fp32", 3: "bf16x6", 4: "f16x3"}
# the regions a pack WRITES in each math mode (the others keep what an earlier mode, or the allocator, left there)
WRITTEN = {0: ("pk_fwd", "pk_bwd"), 3: ("pk_fwd_s", "pk_bwd_s"), 4: ("pk_fwd", "pk_bwd", "pk_fwd_s", "pk_bwd_s", "amax")}
ALWAYS = ("pk_edge", "pk_sbias", "params_pad")

ENGINES = {     # name: kind, in, out, filters, blocks, num_upsample
    "A": ("dn", 1, 1, 32, 1, 1),
    "B": ("sr", 1, 1, 32, 1, 2),
    "C": ("sr", 3, 2, 64, 1, 1),
    "D": ("sr", 1, 1, 48, 1, 1),
    "E": ("dn", 1, 1, 96, 1, 1),
}


def make_engine(name, mode):
    from xmm_superres_denoise.engine import Engine
    kind, ci, co, nf, blocks, nup = ENGINES[name]
    e = Engine(kind, ci, co, nf, blocks, num_upsample=nup)
    e.set_math(MODES[mode])
    return e


def _stream():
    return torch.cuda.current_stream().cuda_stream


def region_call(e, name, dst_ptr, dst_bytes):
    info = ctypes.c_int64(-1)
    rc = e.L.xsd_test_packed_region(e.h, REGION[name] if isinstance(name, str) else name, dst_ptr, dst_bytes, ctypes.byref(info), _stream())
    return rc, info.value


def region(e, name):
    """the region's 32-bit words (int64 words for the table), read through a NaN-guarded device buffer"""
    rc, nbytes = region_call(e, name, None, 0)
    assert rc == 0 and nbytes >= 0 and nbytes % 4 == 0, (name, rc, nbytes)
    if name == "table":
        buf = np.full(nbytes // 8, -1, np.int64)
        assert region_call(e, name, buf.ctypes.data, nbytes)[0] == 0
        return buf
    if nbytes == 0:
        return np.zeros(0, np.uint32)
    g = Guarded(dst=(nbytes // 4,))
    assert region_call(e, name, g.ptr("dst"), nbytes) == (0, nbytes)
    g.check()
    return g.np("dst").view(np.uint32)


# ---- the flat parameter vector of GeneratorRRDB_DN / _SR as the engine lays it out: conv after conv, weight then bias ------------
class Conv:
    def __init__(self, name, cout, cin, tin, off, bwd_scale=1.0, shuffle=0, mfma=True):
        self.name, self.cout, self.cin, self.tin, self.w, self.b = name, cout, cin, tin, off, off + cout * cin * 9
        self.bwd_scale, self.shuffle, self.mfma = bwd_scale, shuffle, mfma
        self.end = self.b + cout


def layout(kind, ci, co, nf, blocks, nup):
    convs, off = [], 0

    def add(*a, **k):
        nonlocal off
        convs.append(Conv(*a, off, **k))
        off = convs[-1].end
    add("conv_first", nf, ci, ci, mfma=False)
    for i in range(blocks):
        for r in range(3):
            for c in range(5):      # conv5's input gradient arrives scaled: 0.2 (x5 * 0.2 + x), and 0.2 * 0.2 for RDB3 (out * 0.2 + x)
                add(f"rrdb.{i}.RDB{r + 1}.conv{c + 1}", nf, nf * (c + 1), nf, bwd_scale=(0.04 if r == 2 else 0.2) if c == 4 else 1.0)
    add("trunk_conv", nf, nf, nf)
    add("conv_last", co, nf, nf, mfma=False)
    if kind == "sr":
        for u in range(nup):
            add(f"upsampling.{3 * u}", 4 * nf, nf, nf, shuffle=1)
        add("HRconv", nf, nf, nf)
    return convs, off


def engine_layouts(name):
    """(real-width convs, n real, padded-width convs, n padded, pad_map): pad_map[i] = place of real parameter i in the padded vector
    (input channel t * nf + k <-> t * nf_pad + k; output channels keep their index)"""
    kind, ci, co, nf, blocks, nup = ENGINES[name]
    nfp = (nf + 31) // 32 * 32
    real, n_real = layout(kind, ci, co, nf, blocks, nup)
    pad, n_pad = layout(kind, ci, co, nfp, blocks, nup)
    pad_map = np.empty(n_real, np.int64)
    for r, p in zip(real, pad):
        ic = np.arange(r.cin)
        icp = ic if r.name == "conv_first" else (ic // nf) * nfp + ic % nf
        oc = np.arange(r.cout)
        pad_map[r.w:r.b] = (p.w + (oc[:, None, None] * p.cin + icp[None, :, None]) * 9 + np.arange(9)[None, None, :]).reshape(-1)
        pad_map[r.b:r.end] = p.b + oc
    return real, n_real, pad, n_pad, pad_map


def shuffle_perm(nf):
    """perm[32 n + c] = the conv channel torch's pixel_shuffle puts at sub-pixel sub = 2 i + j of high-resolution channel 32 q + c, n = sub * P + q"""
    P = nf // 32
    ch = torch.arange(4 * nf, dtype=torch.float32).view(1, 4 * nf, 1, 1)
    ps = torch.nn.functional.pixel_shuffle(ch, 2)[0].numpy().astype(np.int64)       # [nf][i][j]
    return ps.reshape(P, 32, 4).transpose(2, 0, 1).reshape(-1)


def conv_weight(c, vec):
    W = vec[c.w:c.b].reshape(c.cout, c.cin, 9)
    return W[shuffle_perm(c.cin)] if c.shuffle else W      # the packed shuffle conv = the plain pack of W[perm]


def plain_panels(W, scale):
    cout, cin, _ = W.shape
    nn, ns = cout // 32, cin // 32
    fwd = W.reshape(nn, 32, ns, 2, 4, 4, 9).transpose(0, 2, 6, 4, 3, 1, 5)             # (n, co, s, h, j, t, tap) -> [n][s][tap][j][h][co][t]
    bwd = (np.float32(scale) * W)[:, :, ::-1].reshape(nn, 2, 4, 4, ns, 32, 9).transpose(4, 0, 6, 2, 1, 5, 3)   # (n, h, j, t, s, ci, tap') -> [s][n][tap'][j][h][ci][t]
    return fwd.reshape(-1), bwd.reshape(-1)


def fragment_panels(W, scale):
    cout, cin, _ = W.shape
    nn, ns = cout // 32, cin // 32
    fwd = W.reshape(nn, 32, ns, 2, 2, 8, 9).transpose(0, 2, 3, 6, 4, 1, 5)             # (n, m, s, s2, h, j, tap) -> [n][s][s2][tap][h][m][j]
    bwd = (np.float32(scale) * W)[:, :, ::-1].reshape(nn, 2, 2, 8, ns, 32, 9).transpose(4, 0, 1, 6, 2, 5, 3)   # (n, s2, h, j, s, m, tap') -> [s][n][s2][tap'][h][m][j]
    return fwd.reshape(-1), bwd.reshape(-1)


def expected_panels(convs, vec, mode):
    f, b = [], []
    for c in convs:
        if c.mfma:
            pf, pb = (plain_panels if mode == 0 else fragment_panels)(conv_weight(c, vec), c.bwd_scale)
            f.append(pf)
            b.append(pb)
    return np.concatenate(f).astype(np.float32), np.concatenate(b).astype(np.float32)


def split_image(panels, slot):
    """[panel][s2][tap][term h | l][lane][8 x f16] as uint16, plus the mask of the elements whose scaled value is not finite"""
    with np.errstate(all="ignore"):
        h, l, xs = split2(panels, scale_for_amax(slot))
    img = np.stack([h.view(np.uint16).reshape(-1, 64, 8), l.view(np.uint16).reshape(-1, 64, 8)], axis=1)
    return img, ~np.isfinite(xs).reshape(-1, 64, 8)


def expected_edge(convs, vec, ci, co, P):
    first, last = convs[0], next(c for c in convs if c.name == "conv_last")
    Wf = vec[first.w:first.b].reshape(P, 32, ci, 9).transpose(2, 0, 3, 1)      # (q, c, ch, tap) -> [in channel][plane][tap][c]
    Wl = vec[last.w:last.b].reshape(co, P, 32, 9).transpose(0, 1, 3, 2)        # (o, q, c, tap) -> [out channel][plane][tap][c]
    return np.concatenate([Wf.reshape(-1), Wf[:, :, ::-1].reshape(-1), Wl.reshape(-1), Wl[:, :, ::-1].reshape(-1)]).astype(np.float32)


def expected_sbias(convs, vec):
    out = [vec[c.b:c.end][shuffle_perm(c.cin)] for c in convs if c.shuffle]
    return np.concatenate(out).astype(np.float32) if out else np.zeros(0, np.float32)


def fill_index(n):
    assert n < 2 ** 24, "index codes are exact in fp32 only below 2^24"
    return np.arange(1, n + 1, dtype=np.float32)


def fill_random(convs, n, seed):
    rng = np.random.default_rng(seed)
    v = np.empty(n, np.float32)
    for c in convs:
        v[c.w:c.b] = (rng.standard_normal(c.b - c.w) / np.sqrt(9 * c.cin)).astype(np.float32)
        v[c.b:c.end] = (0.1 * rng.standard_normal(c.cout)).astype(np.float32)
    return v


def describe(convs_pad, code):
    """the parameter an index code names, as (conv, oc, ic, tap) of the layout the codes were dealt in"""
    i = int(code) - 1
    for c in convs_pad:
        if c.w <= i < c.b:
            r = i - c.w
            return f"{c.name}.weight[oc {r // (9 * c.cin)}][ic {r // 9 % c.cin}][tap {r % 9}]"
        if c.b <= i < c.end:
            return f"{c.name}.bias[{i - c.b}]"
    return "no parameter (0 = a zero-padded lane)" if code == 0 else f"no parameter (code {code})"


def assert_bits(got_u32, want_f32, what, convs_pad=None, coded=False):
    want = np.ascontiguousarray(want_f32, np.float32).view(np.uint32)
    assert got_u32.size == want.size, f"{what}: {got_u32.size} words, expected {want.size}"
    bad = np.nonzero(got_u32 != want)[0]
    if bad.size:
        i = int(bad[0])
        g, w = got_u32[i:i + 1].view(np.float32)[0], want[i:i + 1].view(np.float32)[0]
        msg = f"{what}: {bad.size} of {want.size} words differ; first at float {i} (panel {i // PANEL}, element {i % PANEL}): got {g!r}, expected {w!r}"
        if coded and convs_pad is not None:
            msg += f"; holds {describe(convs_pad, round(float(g)))}, should hold {describe(convs_pad, round(float(w)))}"
        raise AssertionError(msg)


def pack(e, vec):
    """pack a host vector from a guarded, read-only device copy; returns the Guarded (kept alive: the engine borrows the pointer)"""
    g = Guarded(ro=("params",), params=vec)
    e.pack(g.t["params"])
    torch.cuda.synchronize()
    g.check()
    return g


def check_table(e, name, pad_convs, n_pad):
    kind, ci, co, nf, blocks, nup = ENGINES[name]
    nfp = (nf + 31) // 32 * 32
    t = region(e, "table")
    mf = [c for c in pad_convs if c.mfma]
    nup_e = nup if kind == "sr" else 0
    pk_floats = sum((c.cout // 32) * (c.cin // 32) * PANEL for c in mf)
    assert t[:8].tolist() == [len(mf), nup_e, pad_convs[0].w, next(c for c in pad_convs if c.name == "conv_last").w, nfp // 32,
                              nfp if nfp != nf else 0, pk_floats, n_pad], t[:8]
    assert t.size == 8 + 7 * len(mf) + 2 * nup_e
    pk = sb = 0
    ups = []
    for i, c in enumerate(mf):
        d = t[8 + 7 * i:15 + 7 * i]
        want_scale = int(np.float32(c.bwd_scale).view(np.uint32))
        assert d.tolist() == [c.w, pk, pk, c.cout, c.cin, c.shuffle, want_scale], (c.name, d)
        pk += (c.cout // 32) * (c.cin // 32) * PANEL
        if c.shuffle:
            ups.append([c.b, sb])
            sb += c.cout
    assert t[8 + 7 * len(mf):].reshape(-1, 2).tolist() == ups
    return pk_floats


def check_pack(e, name, mode, vec, coded):
    """every region the pack wrote against the numpy layout, bit for bit"""
    kind, ci, co, nf, blocks, nup = ENGINES[name]
    real, n_real, padc, n_pad, pad_map = engine_layouts(name)
    assert e.nparams == n_real == vec.size
    vp = vec
    if n_pad != n_real:
        vp = np.zeros(n_pad, np.float32)
        vp[pad_map] = vec
    pk_floats = check_table(e, name, padc, n_pad)
    assert_bits(region(e, "params_pad"), vp if n_pad != n_real else np.zeros(0, np.float32), "params_pad", real, coded)
    fwd, bwd = expected_panels(padc, vp, mode)
    assert fwd.size == bwd.size == pk_floats
    src = ("pk_fwd_s", "pk_bwd_s") if mode == 3 else ("pk_fwd", "pk_bwd")       # f16x3 leaves its fp32 fragment panels in pk_fwd / pk_bwd
    got_f, got_b = region(e, src[0]), region(e, src[1])
    assert_bits(got_f, fwd, f"{src[0]} (mode {MODES[mode]})", real, coded)
    assert_bits(got_b, bwd, f"{src[1]} (mode {MODES[mode]})", real, coded)
    if coded:
        # every weight of every packed conv exactly once in the forward panels and exactly once in the dgrad panels (zeros: padded lanes)
        want = np.sort(np.concatenate([vp[c.w:c.b] for c in padc if c.mfma]).astype(np.int64))
        assert np.array_equal(np.sort(got_f.view(np.float32).astype(np.int64)), want)
        scales = np.concatenate([np.full((c.cout // 32) * (c.cin // 32) * PANEL, np.float32(c.bwd_scale)) for c in padc if c.mfma])
        assert np.array_equal(np.sort(np.rint(got_b.view(np.float32).astype(np.float64) / scales.astype(np.float64)).astype(np.int64)), want)
    assert_bits(region(e, "pk_edge"), expected_edge(padc, vp, ci, co, ((nf + 31) // 32)), "pk_edge", real, coded)
    assert_bits(region(e, "pk_sbias"), expected_sbias(padc, vp), "pk_sbias", real, coded)
    if mode == 4:
        check_f16_image(e, fwd, bwd)


def check_f16_image(e, fwd, bwd, loose_nonfinite=False):
    """amax slots = max |panel| as float bits (fmaxf drops NaN); the two-term fp16 images against the numpy restatement with that slot"""
    amax = region(e, "amax").view(np.float32)
    for k, (panels, reg) in enumerate(((fwd, "pk_fwd_s"), (bwd, "pk_bwd_s"))):
        want_slot = np.fmax.reduce(np.abs(panels), initial=np.float32(0))
        assert amax[k:k + 1].view(np.uint32)[0] == np.float32(want_slot).view(np.uint32), f"amax[{k}] = {amax[k]!r}, max |{reg[:6]}| = {want_slot!r}"
        want, odd = split_image(panels, want_slot)
        got = region(e, reg).view(np.uint16).reshape(-1, 2, 64, 8)
        if loose_nonfinite:      # an inf or NaN element: its h is compared as bits where it is inf, its NaN terms by NaN-ness (payloads are not specified)
            gotf, wantf = got.view(np.float16), want.view(np.float16)
            nan_w = np.isnan(wantf)
            assert np.array_equal(np.isnan(gotf), nan_w), f"{reg}: NaN terms are not where the restatement has them"
            assert nan_w[:, 1][odd].all() and not nan_w[~np.stack([odd, odd], 1)].any()
            got, want = np.where(nan_w, 0, got), np.where(nan_w, 0, want)
        else:
            assert not odd.any()
        bad = np.nonzero(got != want)
        if bad[0].size:
            b, t, ln, j = (int(a[0]) for a in bad)
            x = panels.reshape(-1, 64, 8)[b, ln, j]
            raise AssertionError(f"{reg}: {bad[0].size} of {want.size} fp16 words differ from split2; first: block {b} term {'hl'[t]} lane {ln} element {j}, "
                                 f"x = {x!r}, scale {scale_for_amax(want_slot)}: got {got[b, t, ln, j]:#06x}, expected {want[b, t, ln, j]:#06x}")
    return amax


# ---- the five engines x three math modes x two fills -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3, 4])
@pytest.mark.parametrize("name", list(ENGINES))
def test_pack_regions_bit_for_bit(name, mode):
    e = make_engine(name, mode)
    real, n_real, *_ = engine_layouts(name)
    for coded, vec in ((True, fill_index(n_real)), (False, fill_random(real, n_real, 11))):
        g = pack(e, vec)
        check_pack(e, name, mode, vec, coded)
        g.check()


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_padded_width_repack_leaves_nothing_of_the_first_pack(mode):
    """engine D (48 -> 64 filters): a second, different vector packed into the same engine gives a fresh engine's regions"""
    real, n_real, *_ = engine_layouts("D")
    v1, v2 = fill_random(real, n_real, 21), fill_index(n_real)
    e, fresh = make_engine("D", mode), make_engine("D", mode)
    g1 = pack(e, v1)
    first = {r: region(e, r) for r in WRITTEN[mode] + ALWAYS}
    g2 = pack(e, v2)
    gf = pack(fresh, v2)
    for r in WRITTEN[mode] + ALWAYS:
        got, want = region(e, r), region(fresh, r)
        assert np.array_equal(got, want), f"{r}: a repack differs from a fresh engine's pack"
        assert r == "amax" or not np.array_equal(got, first[r]), f"{r}: the second vector changed nothing"
    check_pack(e, "D", mode, v2, True)
    for g in (g1, g2, gf):
        g.check()


def test_pad_gather_takes_exactly_the_real_lanes():
    """pad_params_kernel, gather direction, over all descriptors: index codes in the real lanes of a padded gradient, NaN in every padded lane"""
    real, n_real, padc, n_pad, pad_map = engine_layouts("D")
    e = make_engine("D", 4)
    gpad = np.full(n_pad, np.nan, np.float32)
    gpad[pad_map] = fill_index(n_pad)[pad_map]
    assert np.isnan(gpad).sum() == n_pad - n_real > 0 and np.unique(pad_map).size == n_real
    g = Guarded(ro=("padded",), padded=gpad, real=(n_real,))
    assert e.L.xsd_test_pad_gather(e.h, g.ptr("real"), g.ptr("padded"), _stream()) == 0
    g.check()
    got = g.np("real")
    assert not np.isnan(got).any()
    assert_bits(got.view(np.uint32), gpad[pad_map], "gathered gradient", padc, True)


def test_mode_switches_leave_every_region_as_a_fresh_engine_has_it():
    """f16x3 uses pk_fwd / pk_bwd as fp32 scratch and bf16x6 writes fp32 into pk_fwd_s: 4 -> 0 -> 3 -> 4 on engine B with a pack after each"""
    real, n_real, *_ = engine_layouts("B")
    vec = fill_random(real, n_real, 31)
    e = make_engine("B", 4)
    seen = []
    for mode in (4, 0, 3, 4):
        e.set_math(MODES[mode])
        g = pack(e, vec)
        fresh = make_engine("B", mode)
        gf = pack(fresh, vec)
        now = {r: region(e, r) for r in WRITTEN[mode] + ALWAYS}
        for r, got in now.items():
            assert np.array_equal(got, region(fresh, r)), f"{r} after switching to {MODES[mode]} differs from a fresh engine's"
        check_pack(e, "B", mode, vec, False)
        seen.append(now)
        g.check()
        gf.check()
    for r, got in seen[-1].items():
        assert np.array_equal(got, seen[0][r]), f"{r}: the last f16x3 pack differs from the first"


# ---- the f16x3 image on chosen weights (engine A) ------------------------------------------------------------------------------------
def _fills():
    real, n_real, *_ = engine_layouts("A")
    base = fill_random(real, n_real, 41)
    conv1, conv2, conv5 = real[1], real[2], real[5]
    assert conv5.name == "rrdb.0.RDB1.conv5" and conv5.bwd_scale == 0.2
    out = {}
    out["a_random"] = base.copy()
    v = base.copy()
    v[conv5.w + 1234] = 0.9          # the largest weight sits in a conv5: the dgrad panels hold 0.2 x it, so the two slots (and scales) differ
    out["a_max_in_conv5"] = v
    v = base.copy()
    for c in real:
        v[c.w:c.b] = 0.0
    out["b_zero"] = v
    v = base.copy()
    v[conv5.w + 77] = 2.0 ** 20        # scale 2^-7: every weight under 2^-7 has a subnormal fp16 h term
    out["c_one_huge"] = v
    v = base.copy()
    v[conv2.w + 5] = np.abs(base).max() * np.float32(2.0 ** -30)
    out["d_one_tiny"] = v
    # (e) the maximum is exactly 1.0 in conv1 (scale 2^13 on both sides: no conv5 weight reaches 1 / 0.2 of anything larger); then
    # x * 2^13 = 1024 + n + 0.5 are ties of the h rounding (fp16 ulp 1 in [1024, 2048)), even and odd n, both signs;
    # x * 2^13 = 1024 + (512.25 | 512.75) / 2048 are exact for h and ties of the l rounding (fp16 ulp 0.5 in [512, 1024))
    v = base.copy()
    v[conv1.w] = 1.0
    n = np.arange(200)
    ties_h = (1024.0 + n + 0.5) / 8192.0
    ties_l = (1024.0 + (512.25 + 0.5 * n) / 2048.0) / 8192.0
    t = np.concatenate([ties_h, -ties_h, ties_l, -ties_l]).astype(np.float32)
    assert np.array_equal(t.astype(np.float64), np.concatenate([ties_h, -ties_h, ties_l, -ties_l]))      # exact in fp32
    v[conv2.w + 100:conv2.w + 100 + t.size] = t
    out["e_ties"] = v
    v = base.copy()
    v[conv5.w + 4321] = np.inf
    out["f_one_inf"] = v
    v = base.copy()
    v[conv2.w + 999] = np.nan
    out["g_one_nan"] = v
    return real, out


@pytest.mark.parametrize("fill", ["a_random", "a_max_in_conv5", "b_zero", "c_one_huge", "d_one_tiny", "e_ties", "f_one_inf", "g_one_nan"])
def test_f16x3_image_equals_the_numpy_restatement(fill):
    real, fills = _fills()
    vec = fills[fill]
    e = make_engine("A", 4)
    g = pack(e, vec)
    with np.errstate(all="ignore"):
        fwd, bwd = expected_panels(real, vec, 4)
    nonfinite = fill in ("f_one_inf", "g_one_nan")
    if not nonfinite:      # (the fp32 panels of a NaN weight times bwd_scale carry an unspecified payload)
        assert_bits(region(e, "pk_fwd"), fwd, "pk_fwd")
        assert_bits(region(e, "pk_bwd"), bwd, "pk_bwd")
    amax = check_f16_image(e, fwd, bwd, loose_nonfinite=nonfinite)
    print(f"{fill}: amax {amax[0]!r} {amax[1]!r} scales {scale_for_amax(amax[0])} {scale_for_amax(amax[1])}")
    if fill == "a_max_in_conv5":
        assert amax[0] == np.float32(0.9) and amax[1] < amax[0] and scale_for_amax(amax[0]) != scale_for_amax(amax[1])
    if fill == "b_zero":
        assert amax[0] == 0 and amax[1] == 0 and not region(e, "pk_fwd_s").any() and not region(e, "pk_bwd_s").any()
    if fill == "c_one_huge":      # the case is about subnormal h terms: make sure it has them
        s = scale_for_amax(amax[0])
        sub = (np.abs(fwd) * np.float32(s) < 2.0 ** -14) & (fwd != 0)
        assert amax[0] == 2.0 ** 20 and s == 2.0 ** -7 and sub.mean() > 0.05
    if fill == "e_ties":
        assert amax[0] == 1.0 and amax[1] == 1.0
    if fill == "f_one_inf":
        assert np.isinf(amax[0]) and np.isinf(amax[1])
    if fill == "g_one_nan":       # fmaxf drops the NaN: the slots are those of the other weights, and every other element is case (a)'s with that slot
        assert np.isfinite(amax).all()
    g.check()


# ---- add_channels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,HW", [(2, 3, 35), (1, 1, 1), (3, 8, 256 * 2048 + 77)])
def test_add_channels_bit_for_bit(B, C, HW):
    """dst[b][p] += ((s0 + s1) + s2) ... in fp32, the kernel's order; the last shape needs a second pass of the grid-stride loop
    (2048 x 256 threads); a NaN in one image of src stays in that image"""
    from xmm_superres_denoise.engine import _lib
    L = _lib.load()
    rng = np.random.default_rng(B * 1000 + C)
    src = rng.standard_normal((B, C, HW)).astype(np.float32)
    dst = rng.standard_normal((B, HW)).astype(np.float32)
    nan_at = (B - 1, C - 1, HW // 2)
    src[nan_at] = np.nan
    g = Guarded(ro=("src",), src=src, dst=dst)
    assert L.xsd_test_add_channels(g.ptr("dst"), g.ptr("src"), C, HW, B, _stream()) == 0
    g.check()
    t = np.zeros((B, HW), np.float32)
    for c in range(C):
        t = t + src[:, c]
    want = dst + t
    got = g.np("dst")
    assert np.isnan(got).sum() == 1 and np.isnan(got[nan_at[0], nan_at[2]])
    keep = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])


# ---- refusals: each leaves the destination's NaN fill untouched ---------------------------------------------------------------------------
def test_refusals_copy_nothing():
    from xmm_superres_denoise.engine import Engine, _lib
    L = _lib.load()
    real, n_real, *_ = engine_layouts("A")
    e = make_engine("A", 4)
    g = Guarded(dst=(4096,), src=np.ones(64, np.float32))
    for r in range(len(REGION)):      # before a pack
        assert region_call(e, r, g.ptr("dst"), 4 * 4096)[0] == ERR_STATE
    gp = pack(e, fill_random(real, n_real, 51))
    rc, nbytes = region_call(e, "pk_edge", None, 0)
    assert rc == 0 and nbytes == 4 * 2 * 288 * 2
    assert region_call(e, "pk_edge", g.ptr("dst"), nbytes - 4)[0] == ERR_ARG          # a buffer too small
    assert region_call(e, "amax", g.ptr("dst"), 4)[0] == ERR_ARG
    assert region_call(e, -1, g.ptr("dst"), 4 * 4096)[0] == ERR_ARG                   # an unknown region
    assert region_call(e, len(REGION), g.ptr("dst"), 4 * 4096)[0] == ERR_ARG
    host = np.full(4, -7, np.int64)
    assert region_call(e, "table", host.ctypes.data, 32)[0] == ERR_ARG and (host == -7).all()
    assert L.xsd_test_packed_region(e.h, 0, g.ptr("dst"), 4 * 4096, None, _stream()) == ERR_ARG
    assert L.xsd_test_pad_gather(e.h, g.ptr("dst"), g.ptr("src"), _stream()) == ERR_ARG     # 32 filters: nothing is padded
    wide = Engine("dn", 9, 9, 32, 1)        # nine image channels: a generic-width engine, which has no plane panels
    gw = Guarded(ro=("params",), params=np.zeros(wide.nparams, np.float32))
    wide.pack(gw.t["params"])
    assert region_call(wide, "pk_fwd", g.ptr("dst"), 4 * 4096)[0] == ERR_ARG
    assert L.xsd_test_pad_gather(wide.h, g.ptr("dst"), g.ptr("src"), _stream()) == ERR_ARG
    for C, HW, B in ((0, 8, 1), (1, 0, 1), (1, 8, 0)):
        assert L.xsd_test_add_channels(g.ptr("dst"), g.ptr("src"), C, HW, B, _stream()) == ERR_ARG
    assert L.xsd_test_add_channels(None, g.ptr("src"), 1, 8, 1, _stream()) == ERR_ARG
    assert L.xsd_test_add_channels(g.ptr("dst"), None, 1, 8, 1, _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.t["dst"]).all())
    g.check(untouched=("src",))
    gp.check()
    gw.check()
