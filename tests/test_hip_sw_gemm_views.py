"""The Swin GEMM (sw_gemm_kernel and its bf16x6 twin sw_gemm_s3x_kernel, csrc/sw_kernels.h and sw_gemm_s3x.h) alone in the forms the
SwinFIR, HAT and SwinIR forwards launch it in, through xsd_sw_test_gemm_view (the instance SwinFIR runs) and xsd_swinir_test_gemm_view
(the SW_GEMM_EXT instance): a residual that aliases the output, a residual with a per-image stride, an output that is a column slice
of wider rows, NCHW input with the (x - mean) * img_range affine, O_SHUFFLE, O_NCHW with / img_range + mean, and on the EXT instance
cropped NCHW stores, an NCHW residual, O_SHUFFLE_NCHW and the nearest-2x source.

Every view runs in both math modes under two assertions:
  (i)  against a plain torch restatement in float64 (F.conv2d / matmul, activation, residual, F.pixel_shuffle, the affines, the crop),
       under the project's bar: rms and max-relative error at most 2 x those of the same restatement in fp32 on the device;
  (ii) BITWISE against a composition: the plain entry's token-major result for the same operands (xsd_sw_test_gemm; on the EXT instance
       the view entry in its plain form, or xsd_swinir_test_nearest_conv), then + res, / range + mean and the permutation as single
       IEEE operations in torch fp32 on the host, in the kernel's order.  The input affine is fed to the plain entry as
       (x - mean) * range computed in torch.
The output buffer is sentinel-filled between guard bands and compared whole: every element that should be written is written, nothing
else changes.  Each view also runs twice (same bits), image by image (B = 3 equals three B = 1 runs) and with a NaN in one image's
input or residual (the other images keep their bits).

The tile is 128 rows x 64 columns; a K round is 16 (fp32) or 32 (bf16x6).  B = 3 images of 7 x 9 give M = 189: the first row tile holds
parts of three images and the second is ragged.

Measured on the MI355X: every (ii) is exact, in both modes, on both instances, and every (i) is met.  The three O_SHUFFLE cases
(a 3x3 conv from 4 channels, K = 36) are what made sw_gemm_kernel cut sums of K <= 48 into fmaf chains of 4: with its chains of 16
"shuffle r 2, N 20" and "shuffle r 2, N 132" sat at 2.46 x and 2.34 x the max-relative error of torch's fp32 conv, which is all but
correctly rounded at that size (rms 4.47e-08), and "shuffle r 3, N 72" at 1.98 x.  They are now at 1.17 x, 1.35 x and 1.51 x (rms
1.29 x to 1.31 x); the stores were exact (ii) before and after.  DESIGN.md section 25 and profiles/r23_gemm_small_k_rounding.txt
have the record."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SENT = -12345.0
GUARD = 4096
MATHS = ("fp32", "bf16x6")


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _within_2x_of_fp32(y, y32, y64, what):
    """the project's bar, printed; returns (met, figures)"""
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e} | ratio rms "
          f"{rms / rms32:.2f} max-rel {mx / mx32:.2f}")
    return rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


def case(name, **kw):
    c = dict(name=name, ext=False, conv3=True, B=3, H=7, W=9, a="tok", imean=None, irange=1.0, act=None, slope=0.0, res=None, omode="tok",
             ldy=None, off=0, r=1, omean=None, orange=1.0, cH=0, cW=0, up2=False)
    c.update(kw)
    if c["ldy"] is None:
        c["ldy"] = c["N"]
    return c


def _osize(c):
    u = 2 if c["up2"] else 1
    return u * c["H"], u * c["W"]


def _per_image(c):
    oH, oW = _osize(c)
    r = c["r"]
    if c["omode"] == "tok":
        return oH * oW * c["ldy"]
    if c["omode"] == "shuffle":
        return oH * oW * c["N"]
    if c["omode"] == "nchw":
        return c["N"] * (c["cH"] or oH) * (c["cW"] or oW)
    return c["N"] // (r * r) * c["cH"] * c["cW"]


def _operands(c):
    """the case's operands on the host: x in the layout the case names ([B, H, W, cin] or NCHW), w, bias, the residual as [B, oH, oW, N]"""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])) * 7919 + c["N"])
    B, H, W, cin, N = c["B"], c["H"], c["W"], c["cin"], c["N"]
    oH, oW = _osize(c)
    x = torch.randn((B, cin, H, W) if c["a"] == "nchw" else (B, H, W, cin), generator=g)
    if c["imean"] is not None:
        x = x * 0.3 + 0.4            # image-like values around the mean that is subtracted
    K = cin * (9 if c["conv3"] else 1)
    w = torch.randn((N, cin, 3, 3) if c["conv3"] else (N, cin), generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    res = torch.randn(B, oH, oW, N, generator=g) if c["res"] else None
    return x, w, b, res


def _vec(v, dtype, device):
    return None if v is None else torch.tensor(v, dtype=dtype, device=device)


def _restate(c, x, w, b, dtype):
    """act(A W^T + bias) as [B, oH, oW, N] in `dtype` on the device: the reference of (i)"""
    B, H, W, cin, N = x.shape[0], c["H"], c["W"], c["cin"], c["N"]
    xd, wd, bd = x.cuda().to(dtype), w.cuda().to(dtype), b.cuda().to(dtype)
    if c["conv3"]:
        xn = xd if c["a"] == "nchw" else xd.permute(0, 3, 1, 2)
        if c["imean"] is not None:
            xn = (xn - _vec(c["imean"], dtype, "cuda").view(1, -1, 1, 1)) * c["irange"]
        if c["up2"]:
            xn = F.interpolate(xn, scale_factor=2, mode="nearest")
        v = F.conv2d(xn.contiguous(), wd, bd, padding=1).permute(0, 2, 3, 1)
    else:
        v = (xd.reshape(-1, cin) @ wd.T + bd).view(B, H, W, N)
    if c["act"] == "gelu":
        v = F.gelu(v)
    elif c["act"] == "lrelu":
        v = F.leaky_relu(v, c["slope"])
    return v


def _finish(c, v, res):
    """what follows the activation, in the kernel's order: + res, then / range + mean, then the permutation and the crop; v and res are
    [B, oH, oW, N].  Returns the whole y buffer as [B, floats per image] with the sentinel where nothing is stored."""
    B, N, r = v.shape[0], c["N"], c["r"]
    oH, oW = _osize(c)
    if res is not None:
        v = v + res
    if c["omode"] == "tok":
        out = torch.full((B, oH * oW, c["ldy"]), SENT, dtype=v.dtype, device=v.device)
        out[:, :, c["off"]:c["off"] + N] = v.reshape(B, oH * oW, N)
        return out.reshape(B, -1)
    t = v.permute(0, 3, 1, 2)
    if c["omode"] in ("shuffle", "shuffle_nchw"):
        t = F.pixel_shuffle(t, r)
    if c["omode"] == "shuffle":
        return t.permute(0, 2, 3, 1).reshape(B, -1)
    # a one-element tensor, not a Python number: torch may multiply by the reciprocal of a scalar divisor
    t = t / torch.full((1,), c["orange"], dtype=v.dtype, device=v.device) + _vec(c["omean"], v.dtype, v.device).view(1, -1, 1, 1)
    if c["cH"]:
        t = t[:, :, :c["cH"], :c["cW"]]
    return t.reshape(B, -1)


def _launch(c, math, x, w, b, res):
    """one launch of the view on the device, the y buffer between guard bands; returns it whole as [B, floats per image] on the host"""
    from xmm_superres_denoise.engine import sw_gemm_view
    B, N = x.shape[0], c["N"]
    oH, oW = _osize(c)
    oHW, per = oH * oW, _per_image(c)
    buf = torch.full((2 * GUARD + B * per,), SENT, device="cuda")
    ybuf = buf[GUARD:GUARD + B * per]
    kw = {}
    if c["res"] == "alias":                 # in place: the residual is what the output rows hold
        ybuf.view(B, oHW, c["ldy"])[:, :, c["off"]:c["off"] + N] = res.cuda().reshape(B, oHW, N)
        kw = dict(res=ybuf[c["off"]:], rbs=oHW * c["ldy"] if c["conv3"] else 0, rps=c["ldy"])
    elif c["res"] == "strided":             # a tensor of its own, images 24 floats apart (token rows are one image: dense there)
        gap = 24 if c["conv3"] else 0
        rd = torch.full((B, oHW * N + gap), SENT, device="cuda")
        rd[:, :oHW * N] = res.cuda().reshape(B, -1)
        kw = dict(res=rd, rbs=(oHW * N + gap) if c["conv3"] else 0, rps=N)
    elif c["res"] == "nchw":
        kw = dict(res=res.cuda().permute(0, 3, 1, 2).contiguous(), rbs=N * oHW, rnchw=True)
    sw_gemm_view(x.cuda().contiguous(), w.cuda(), ybuf[c["off"]:], conv3=c["conv3"], B=B, H=c["H"], W=c["W"], cin=c["cin"], N=N, ext=c["ext"],
                 a_nchw=c["a"] == "nchw", lda=c["cin"], imean=_vec(c["imean"], torch.float32, "cuda"), irange=c["irange"], bias=b.cuda(),
                 act=c["act"], slope=c["slope"], omode=c["omode"], ldy=c["ldy"] if c["omode"] == "tok" else 0, r=c["r"],
                 omean=_vec(c["omean"], torch.float32, "cuda"), orange=c["orange"], math=math, cH=c["cH"], cW=c["cW"], up2=c["up2"], **kw)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + B * per:] == SENT).all()), (c["name"], math, "guard band written")
    return ybuf.view(B, per).cpu()


def _plain(c, math, x, w, b):
    """the plain entry's token-major result for the same operands as [B, oH, oW, N] on the host: contiguous token-major input, no
    residual, a dense token-major store.  On the EXT instance the plain entry is the view entry in that form (it is pinned against
    float64 by its own cases below), and xsd_swinir_test_nearest_conv for the nearest-2x source."""
    from xmm_superres_denoise.engine import _lib, sw_gemm_view
    from xmm_superres_denoise.engine.engine import SW_ACT, SW_MATH
    B, H, W, cin, N = x.shape[0], c["H"], c["W"], c["cin"], c["N"]
    oH, oW = _osize(c)
    if c["a"] == "nchw":
        if c["imean"] is not None:
            x = (x - _vec(c["imean"], torch.float32, "cpu").view(1, -1, 1, 1)) * c["irange"]
        x = x.permute(0, 2, 3, 1)
    xd, wd, bd = x.contiguous().cuda(), w.cuda(), b.cuda()
    y = torch.full((B * oH * oW, N), SENT, device="cuda")
    L, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    if c["up2"]:
        assert c["act"] == "lrelu"
        _lib.check(L.xsd_swinir_test_nearest_conv(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H, W, cin, N, c["slope"],
                                                  SW_MATH[math], stream))
    elif c["ext"]:
        sw_gemm_view(xd, wd, y, conv3=c["conv3"], B=B, H=H, W=W, cin=cin, N=N, ext=True, lda=cin, bias=bd, act=c["act"], slope=c["slope"],
                     ldy=N, math=math)
    else:
        _lib.check(L.xsd_sw_test_gemm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), int(c["conv3"]), B, H, W, cin, N, N,
                                      SW_ACT[c["act"]], c["slope"], SW_MATH[math], stream))
    torch.cuda.synchronize()
    return y.view(B, oH, oW, N).cpu()


def _is_plain(c):
    return c["ext"] and not c["up2"] and c["a"] == "tok" and c["res"] is None and c["omode"] == "tok" and c["ldy"] == c["N"]


def _check_view(c):
    x, w, b, res = _operands(c)
    B = c["B"]
    written = _finish(c, torch.zeros(B, *_osize(c), c["N"]), None) != SENT
    ref64 = _finish(c, _restate(c, x, w, b, torch.float64), None if res is None else res.cuda().double()).cpu()
    ref32 = _finish(c, _restate(c, x, w, b, torch.float32), None if res is None else res.cuda()).cpu()
    bars = []
    for math in MATHS:
        what = f"GEMM view {'ext ' if c['ext'] else ''}{c['name']} {math}"
        y = _launch(c, math, x, w, b, res)
        # (i) float64, on the elements that are stored; asserted last, so that a miss of the bar hides nothing of what follows
        bars.append(_within_2x_of_fp32(y[written].numpy(), ref32[written].numpy(), ref64[written].numpy(), what))
        # (ii) the composition, on the whole buffer: stored elements bit for bit, the sentinel everywhere else
        if not _is_plain(c):
            want = _finish(c, _plain(c, math, x, w, b), res)
            same = want.view(torch.int32) == y.view(torch.int32)
            assert bool(same.all()), (what, "composition", int((~same).sum()), float((want - y).abs().max()))
        else:
            assert bool((y[~written] == SENT).all()) and not bool((y[written] == SENT).any()), what
        # two runs
        assert torch.equal(_launch(c, math, x, w, b, res).view(torch.int32), y.view(torch.int32)), (what, "second run")
        if B == 1:
            continue
        # image by image
        for i in range(B):
            yi = _launch(c, math, x[i:i + 1], w, b, None if res is None else res[i:i + 1])
            assert torch.equal(yi.view(torch.int32), y[i:i + 1].view(torch.int32)), (what, "B = 1 run of image", i)
        # a NaN in image 1's input, then in its residual: the other images keep their bits
        poisoned = [("input", x.clone(), res)]
        poisoned[0][1][(1,) + tuple(s // 2 for s in x.shape[1:])] = float("nan")
        if res is not None:
            rn = res.clone()
            rn[1, 1, 2, c["N"] // 2] = float("nan")
            poisoned.append(("residual", x, rn))
        for where, xn, rn in poisoned:
            yn = _launch(c, math, xn, w, b, rn)
            assert bool(torch.isnan(yn[1]).any()), (what, where)
            for i in range(B):
                if i != 1:
                    assert torch.equal(yn[i].view(torch.int32), y[i].view(torch.int32)), (what, "NaN in the", where, "reached image", i)
    assert all(ok for ok, _ in bars), [f for ok, f in bars if not ok]


MEAN3 = (0.4, -0.2, 0.7)
CASES = [
    # ---- the instance SwinFIR runs ----
    case("token, in-place residual, 130 x 20 x 70", conv3=False, B=1, H=1, W=130, cin=20, N=70, res="alias"),
    case("token, in-place residual, 5 x 7 x 33", conv3=False, B=1, H=1, W=5, cin=7, N=33, res="alias"),
    case("token, in-place residual, 189 x 20 x 70", conv3=False, cin=20, N=70, res="alias"),
    case("token, column slice 12 of 24", conv3=False, cin=10, N=12, ldy=24, off=12),
    case("conv 12 -> 20, strided residual, ldy 40, lrelu", cin=12, N=20, res="strided", ldy=40, act="lrelu", slope=0.2),
    case("conv 12 -> 20, strided residual, ldy 40", cin=12, N=20, res="strided", ldy=40),
    case("conv from NCHW, 3 channels, range 1", B=2, H=5, W=7, cin=3, N=16, a="nchw", imean=MEAN3, irange=1.0),
    case("conv from NCHW, 3 channels, range 255", B=2, H=5, W=7, cin=3, N=16, a="nchw", imean=MEAN3, irange=255.0),
    case("conv from NCHW, 1 channel, range 255", B=2, H=5, W=7, cin=1, N=16, a="nchw", imean=(0.3,), irange=255.0),
    case("shuffle r 2, N 20", cin=4, N=20, omode="shuffle", r=2),
    case("shuffle r 3, N 72", cin=4, N=72, omode="shuffle", r=3),
    case("shuffle r 2, N 132", cin=4, N=132, omode="shuffle", r=2),
    # either side of sw_gemm_kernel's K <= 48 instance: K = 45 runs in fmaf chains of 4, K = 54 in chains of 16
    case("shuffle r 2, N 20, 5 channels (K 45)", cin=5, N=20, omode="shuffle", r=2),
    case("shuffle r 2, N 20, 6 channels (K 54)", cin=6, N=20, omode="shuffle", r=2),
    case("conv 6 -> 20 (K 54), token store", cin=6, N=20),
    case("NCHW store, 8 -> 1", cin=8, N=1, omode="nchw", omean=(0.3,), orange=255.0),
    case("NCHW store, 8 -> 3", cin=8, N=3, omode="nchw", omean=MEAN3, orange=255.0),
    case("NCHW store, 3 -> 3", cin=3, N=3, omode="nchw", omean=MEAN3, orange=255.0),
    case("NCHW store, 3 -> 1", cin=3, N=1, omode="nchw", omean=(0.3,), orange=255.0),
    # ---- SwinIR's SW_GEMM_EXT instance ----
    case("plain token 130 x 20 x 70", ext=True, conv3=False, B=1, H=1, W=130, cin=20, N=70),
    case("plain token 5 x 7 x 33, gelu", ext=True, conv3=False, B=1, H=1, W=5, cin=7, N=33, act="gelu"),
    case("plain conv 2 x 5 x 7, 12 -> 33", ext=True, B=2, H=5, W=7, cin=12, N=33),
    case("plain conv 3 x 6 x 6, 1 -> 16", ext=True, B=3, H=6, W=6, cin=1, N=16),
    case("NCHW store cropped 8 x 12 -> 7 x 10", ext=True, B=2, H=8, W=12, cin=8, N=3, omode="nchw", omean=MEAN3, orange=255.0, cH=7, cW=10),
    case("NCHW store, NCHW residual", ext=True, B=2, H=8, W=12, cin=8, N=3, omode="nchw", omean=MEAN3, orange=255.0, res="nchw"),
    case("NCHW store, NCHW residual, cropped", ext=True, B=2, H=8, W=12, cin=8, N=3, omode="nchw", omean=MEAN3, orange=255.0, res="nchw",
         cH=7, cW=10),
] + [
    case(f"shuffle into NCHW r {r}, C {C}{', cropped' if crop else ''}", ext=True, B=2, H=5, W=6, cin=8, N=r * r * C, omode="shuffle_nchw", r=r,
         omean=MEAN3[:C], orange=255.0, cH=5 * r - (2 if crop else 0), cW=6 * r - (1 if crop else 0))
    for r in (2, 3, 4) for C in (1, 3) for crop in (True, False)
] + [
    case("nearest-2x source, NCHW residual, cropped 8 x 10 -> 7 x 9", ext=True, B=2, H=4, W=5, cin=8, N=3, up2=True, act="lrelu", slope=0.2,
         omode="nchw", omean=MEAN3, orange=255.0, res="nchw", cH=7, cW=9),
]


@pytest.mark.parametrize("c", CASES, ids=[("ext " if c["ext"] else "") + c["name"] for c in CASES])
def test_view(c):
    _check_view(c)


@pytest.mark.parametrize("math", MATHS)
def test_bf16x6_staging_paths_agree(math):
    """sw_gemm_s3x_kernel picks 16-byte vector staging or per-element staging at run time from cin % 4, the strides and the pointer's
    alignment.  The same 189 x 20 matrix through an aligned base with lda = 20 (vector) and through a base shifted by one float with
    lda = 21 (per element; no forward launches this form) must give the same bits, in fp32 too, and meet the float64 bar."""
    from xmm_superres_denoise.engine import sw_gemm_view
    M, K, N = 189, 20, 70
    g = torch.Generator().manual_seed(2021)
    a, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    ad, wd, bd = a.cuda(), w.cuda(), b.cuda()
    assert ad.data_ptr() % 16 == 0
    big = torch.full((1 + M * 21,), SENT, device="cuda")
    shifted = big[1:].view(M, 21)
    shifted[:, :K] = ad
    assert shifted.data_ptr() % 16 == 4
    outs = []
    for src, lda in ((ad, K), (shifted, 21)):
        y = torch.full((M + 3, N + 5), SENT, device="cuda")
        sw_gemm_view(src, wd, y, conv3=False, B=3, H=7, W=9, cin=K, N=N, lda=lda, bias=bd, ldy=N + 5, math=math)
        assert bool((y[M:] == SENT).all()) and bool((y[:, N:] == SENT).all())
        outs.append(y[:M, :N].clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref64 = (ad.double() @ wd.double().T + bd.double()).cpu().numpy()
    ok, figures = _within_2x_of_fp32(outs[1].cpu().numpy(), (ad @ wd.T + bd).cpu().numpy(), ref64, f"GEMM view shifted base, lda 21, {math}")
    assert ok, figures


def test_refusals_from_python_name_their_argument():
    from xmm_superres_denoise.engine import XsdError, sw_gemm_view
    a, w, y = torch.zeros(6, 4, device="cuda"), torch.zeros(8, 4, device="cuda"), torch.zeros(6, 8, device="cuda")
    ok = dict(conv3=False, B=1, H=1, W=6, cin=4, N=8, lda=4, ldy=8)
    sw_gemm_view(a, w, y, **ok)
    for kw, msg in ((dict(act="relu"), "unknown activation 'relu'"), (dict(math="tf32"), "unknown math mode 'tf32'"),
                    (dict(omode="nhwc"), "unknown omode 'nhwc'"), (dict(bias=torch.zeros(7, device="cuda")), "bias has 7 elements for 8"),
                    (dict(bias=torch.zeros(8)), "bias must be a float32 CUDA"), (dict(res=torch.zeros(6, 8, device="cuda", dtype=torch.float64)),
                                                                                  "res must be a float32 CUDA"),
                    (dict(imean=torch.zeros(3, device="cuda")), "imean has 3 elements for 4"),
                    (dict(omode="nchw", omean=torch.zeros(3, device="cuda")), "omean has 3 elements for 8")):
        with pytest.raises(XsdError, match=msg):
            sw_gemm_view(a, w, y, **dict(ok, **kw))
    with pytest.raises(XsdError, match="w .* is not the contiguous"):
        sw_gemm_view(a, torch.zeros(8, 5, device="cuda"), y, **ok)
    with pytest.raises(XsdError, match="y is missing"):
        sw_gemm_view(a, w, None, **ok)


def test_refusals_from_the_library_name_their_argument():
    from xmm_superres_denoise.engine import _lib
    L = _lib.load()
    p = torch.zeros(4096, device="cuda")
    ptr = p.data_ptr()

    def view(**kw):
        v = dict(conv3=1, B=1, H=4, W=4, cin=4, N=8, a=ptr, lda=4, w=ptr, y=ptr, ldy=8, r=1, orange=1.0)
        v.update(kw)
        return _lib.XsdSwGemmView(**v)

    before = p.clone()
    both = (L.xsd_sw_test_gemm_view, L.xsd_swinir_test_gemm_view)
    for entries, v, msg in (
            (both, view(a=None), b"a is null"), (both, view(w=None), b"w is null"), (both, view(y=None), b"y is null"),
            (both, view(omode=2, omean=None), b"omean is null"),
            (both, view(omode=1, r=2, N=18), b"N = 18 is no multiple of r^2"), (both, view(omode=1, r=3, N=8), b"N = 8 is no multiple of r^2"),
            (both, view(N=0), b"bad shape"), (both, view(ldy=7), b"ldy 7 is less than N"), (both, view(lda=5), b"lda 5"),
            (both, view(conv3=0, lda=3), b"lda 3"), (both, view(act=3), b"act 3"), (both, view(math=4), b"math 4"), (both, view(omode=4), b"omode 4"),
            (both, view(conv3=0, omode=1, r=2), b"need conv3"), (both, view(conv3=0, a_nchw=1), b"need conv3"),
            (both, view(conv3=0, res=ptr, rbs=8, rps=8), b"rbs 8 on token rows"), (both, view(omode=2, omean=ptr, orange=0.0), b"orange must be positive"),
            (both[:1], view(rnchw=1, res=ptr), b"belong to xsd_swinir_test_gemm_view"), (both[:1], view(up2=1), b"belong to xsd_swinir_test_gemm_view"),
            (both[:1], view(omode=2, omean=ptr, cH=3, cW=3), b"belong to xsd_swinir_test_gemm_view"),
            (both[:1], view(omode=3, omean=ptr, r=2, cH=8, cW=8), b"belong to xsd_swinir_test_gemm_view"),
            (both[1:], view(omode=2, omean=ptr, cH=5, cW=4), b"the crop cH 5 x cW 4 is larger than the 4 x 4 result"),
            (both[1:], view(omode=2, omean=ptr, cH=8, cW=9, up2=1), b"the crop cH 8 x cW 9 is larger than the 8 x 8 result"),
            (both[1:], view(omode=3, omean=ptr, r=2, cH=8, cW=9), b"the crop cH 8 x cW 9 is larger than the 8 x 8 result"),
            (both[1:], view(omode=3, omean=ptr, r=2), b"omode 3 needs cH and cW"), (both[1:], view(omode=2, omean=ptr, cH=3), b"both or neither"),
            (both[1:], view(ldy=8, cH=2, cW=2), b"cH and cW go with omode 2 or 3"), (both[1:], view(a_nchw=1, up2=1), b"a_nchw with up2")):
        for fn in entries:
            assert fn(ctypes.byref(v), None) != 0 and msg in L.xsd_last_error(), (msg, L.xsd_last_error())
    for fn in both:
        assert fn(None, None) != 0 and b"the view is null" in L.xsd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(p, before)          # a refused call launches nothing
