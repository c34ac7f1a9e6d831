"""The FourierUnit's FFT (sw_fft_kernel, csrc/swinfir.hip) on its own at every radix pass: 7, 11 and 13 alone and first, a radix twice in
one length (so that the twiddle tw[r k step] between two passes of the same radix is not 1), mixed chains in the factoriser's order,
all six primes in one length, the 4096 limit (one line per workgroup, exactly 64 KiB of LDS), a last line block that is partly empty,
and the degenerate lengths 1, 2 and 3 with the zero-stage path.

Forward is rfftn(ortho); inverse is x + irfftn(s=(H, W), ortho) of a random spectrum that is NOT Hermitian along H and has non-zero
imaginary parts at DC and Nyquist.  The reference is torch.fft in float64; the yardstick is torch.fft in float32 on the CPU on the same
input.  Bars: rms error <= 2 x the yardstick's; max error over max |ref| <= max(5e-7, 2 x the yardstick's); where the yardstick is
exactly 0 the result must be exact.  The bars rest on a float32 numpy emulation of the kernel's Stockham passes (same radix order,
table twiddles made in double), forward only: rms 0.91 to 1.31 and max-relative 0.83 to 1.54 times torch.fft float32's, worst
max-relative 2.0e-7 (at 2197 x 3), which is why the max bar has an absolute floor and the rms bar has none.

Measured on the MI355X: see the table in DESIGN.md section 25."""
import numpy as np
import pytest
import torch

import util_hip as U

pytestmark = pytest.mark.gpu

ALONE = [(1, 7, 11, 3), (2, 11, 7, 2), (1, 13, 5, 1)]
TWICE = [(1, 49, 121, 2), (1, 169, 25, 2), (1, 9, 27, 2)]
MIXED = [(1, 14, 22, 3), (1, 28, 44, 2), (1, 77, 91, 2), (2, 56, 88, 5)]
PRIMES = [(1, 3003, 2, 1), (1, 2, 3003, 1)]
LIMIT = [(1, 4096, 2, 3), (1, 2, 4096, 3), (1, 2, 4095, 2)]
BLOCKS = [(1, 2048, 4, 3), (1, 273, 4, 17)]        # 2 lines per workgroup with odd C2; 15 lines with 2 of 15 valid in the second block
DEGENERATE = [(1, 1, 1, 1), (2, 1, 8, 3), (2, 8, 1, 3), (1, 2, 2, 1), (1, 3, 3, 2), (1, 1, 3, 20)]
SHAPES = ALONE + TWICE + MIXED + PRIMES + LIMIT + BLOCKS + DEGENERATE


@pytest.fixture(scope="module")
def eng():
    from xmm_superres_denoise.engine import SwinFIREngine
    return SwinFIREngine((16, 16), (1, 1), 1, 16, [1], [2], 4, 4.0, True, None, False, True, 2, 1.0, "pixelshuffle", "SFB")


def _inputs(B, H, W, C2):
    g = torch.Generator().manual_seed(100003 * H + 101 * W + C2)
    return torch.randn(B, H, W, C2, generator=g), torch.randn(B, H, W // 2 + 1, C2, 2, generator=g)


def _rfftn(x):
    r = torch.fft.rfftn(x, dim=(1, 2), norm="ortho")
    return torch.stack((r.real, r.imag), dim=-1)


def _x_plus_irfftn(x, s):
    return x + torch.fft.irfftn(torch.complex(s[..., 0], s[..., 1]), s=tuple(x.shape[1:3]), dim=(1, 2), norm="ortho")


def _errs(y, ref):
    e = (y.double() - ref).abs()
    return float(e.pow(2).mean().sqrt()), float(e.max() / ref.abs().max())


def _bar(y, y32, y64, what):
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    ratio = (f"{rms / rms32:.2f}", f"{mx / mx32:.2f}") if rms32 > 0 and mx32 > 0 else ("-", "-")
    print(f"FFT {what}: engine rms {rms:.3e} max-rel {mx:.3e} | torch.fft fp32 rms {rms32:.3e} max-rel {mx32:.3e} | ratio rms {ratio[0]} "
          f"max-rel {ratio[1]}")
    assert y.shape == y64.shape and bool(torch.isfinite(y).all()), what
    if rms32 == 0.0:
        assert rms == 0.0, (what, rms)
        return
    assert rms <= 2 * rms32, (what, rms, rms32)
    assert mx <= max(5e-7, 2 * mx32), (what, mx, mx32)


@pytest.mark.parametrize("B,H,W,C2", SHAPES)
def test_every_radix_against_torch_fft(eng, B, H, W, C2):
    x, s = _inputs(B, H, W, C2)
    spec = eng.fourier_pair(x.cuda()).cpu()
    _bar(spec, _rfftn(x), _rfftn(x.double()), f"{B} x {H} x {W} x {C2} rfftn")
    back = eng.fourier_pair(x.cuda(), s.cuda()).cpu()
    _bar(back, _x_plus_irfftn(x, s), _x_plus_irfftn(x.double(), s.double()), f"{B} x {H} x {W} x {C2} x + irfftn")


ISO = (2, 14, 22, 5)       # five channels share one workgroup's LDS in both axes


def _others_equal(got, clean, b, c, what):
    """got[b, :, :, c] is NaN everywhere, every other (image, channel) is bitwise the clean run"""
    assert bool(torch.isnan(got[b, :, :, c]).all()), what
    keep = torch.ones(got.shape[0], got.shape[3], dtype=torch.bool)
    keep[b, c] = False
    for bb in range(got.shape[0]):
        for cc in range(got.shape[3]):
            if keep[bb, cc]:
                assert torch.equal(got[bb, :, :, cc], clean[bb, :, :, cc]), (what, bb, cc)


def test_a_nan_stays_inside_its_image_and_channel(eng):
    x, s = _inputs(*ISO)
    x, s = x.cuda(), s.cuda()
    clean_f, clean_i = eng.fourier_pair(x), eng.fourier_pair(x, s)
    xn = x.clone()
    xn[1, 5, 7, 3] = float("nan")
    _others_equal(eng.fourier_pair(xn), clean_f, 1, 3, "forward, NaN in x")
    sn = s.clone()
    sn[1, 3, 2, 3, 0] = float("nan")
    _others_equal(eng.fourier_pair(x, sn), clean_i, 1, 3, "inverse, NaN in the spectrum")


@pytest.mark.parametrize("shape", [(2, 1, 8, 3), (1, 1, 3, 20)])
def test_imaginary_parts_of_dc_and_nyquist_do_not_enter(eng, shape):
    """torch's C2R never reads them, and the kernel replaces them by 0.  In exact arithmetic they reach only the imaginary output that
    the C2R pass discards, so the comparison with torch.fft cannot see whether they are dropped (the mutant that keeps them passes
    it); a NaN there can.  H = 1, where the column pass is the zero-stage path and leaves an imaginary NaN imaginary."""
    x, s = _inputs(*shape)
    W = shape[2]
    sn = s.clone()
    sn[:, :, 0, :, 1] = float("nan")
    if W % 2 == 0:
        sn[:, :, W // 2, :, 1] = float("nan")
    assert torch.equal(eng.fourier_pair(x.cuda(), sn.cuda()), eng.fourier_pair(x.cuda(), s.cuda()))


@pytest.mark.parametrize("shape", [ISO, (2, 56, 88, 5), (2, 273, 4, 17)])
def test_two_runs_and_two_batch_sizes_give_the_same_bits(eng, shape):
    x, s = _inputs(*shape)
    x, s = x.cuda(), s.cuda()
    f, i = eng.fourier_pair(x), eng.fourier_pair(x, s)
    assert torch.equal(eng.fourier_pair(x), f) and torch.equal(eng.fourier_pair(x, s), i)
    for b in range(shape[0]):
        assert torch.equal(eng.fourier_pair(x[b:b + 1].contiguous()), f[b:b + 1]), b
        assert torch.equal(eng.fourier_pair(x[b:b + 1].contiguous(), s[b:b + 1].contiguous()), i[b:b + 1]), b


@pytest.mark.parametrize("B,H,W,C2", [ISO, (1, 273, 4, 17), (1, 2048, 4, 3), (1, 4096, 2, 3), (1, 2, 4095, 2), (1, 1, 3, 20), (1, 1, 1, 1)])
def test_nothing_is_written_outside(eng, B, H, W, C2):
    """forward: x is read only, every element of [B][H][W/2+1][2 C2] is written and no guard band is touched.  Inverse: the entry
    overwrites the spectrum it is given (its contract) and adds into x; both stay inside their extents."""
    x, s = _inputs(B, H, W, C2)
    stream = torch.cuda.current_stream().cuda_stream
    g = U.Guarded(ro=("x",), x=x.numpy(), spec=(B, H, W // 2 + 1, C2, 2))
    assert eng.L.xsd_swinfir_test_fft(eng.h, g.ptr("x"), g.ptr("spec"), B, H, W, C2, 0, stream) == 0
    torch.cuda.synchronize()
    g.check()
    assert bool(torch.isfinite(g.t["spec"]).all())
    assert torch.equal(g.t["spec"], eng.fourier_pair(x.cuda()))
    g = U.Guarded(x=x.numpy(), spec=s.numpy())
    assert eng.L.xsd_swinfir_test_fft(eng.h, g.ptr("x"), g.ptr("spec"), B, H, W, C2, 1, stream) == 0
    torch.cuda.synchronize()
    g.check()
    assert bool(torch.isfinite(g.t["x"]).all()) and bool(torch.isfinite(g.t["spec"]).all())
    assert torch.equal(g.t["x"], eng.fourier_pair(x.cuda(), s.cuda()))


def _supported(n):
    for p in (2, 3, 5, 7, 11, 13):
        while n > 1 and n % p == 0:
            n //= p
    return n == 1


def test_supported_lengths_are_the_13_smooth_ones_up_to_4096():
    from xmm_superres_denoise.engine import fft_size_supported
    for n in range(-1, 4201):
        assert fft_size_supported(n) == (1 <= n <= 4096 and _supported(n)), n


@pytest.mark.parametrize("n", [17, 4097, 8192])
def test_unsupported_lengths_are_refused_by_name(eng, n):
    from xmm_superres_denoise.engine import XsdError
    for shape in ((1, n, 2, 1), (1, 2, n, 1)):
        x = torch.zeros(shape, device="cuda")
        with pytest.raises(XsdError, match=rf"FFT size {n} is not supported"):
            eng.fourier_pair(x)
        with pytest.raises(XsdError, match=rf"FFT size {n} is not supported"):
            eng.fourier_pair(x, torch.zeros(shape[0], shape[1], shape[2] // 2 + 1, 1, 2, device="cuda"))
