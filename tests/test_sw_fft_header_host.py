"""The FourierUnit's FFT passes live in one header, csrc/sw_fft.h, which the fused SwinFIR forward includes the way it includes
sw_kernels.h: the kernel, its launcher, the factoriser and the twiddle table, so that a second translation unit can compile the very
same passes.  Pinned without a device: where the code is, that swinfir.hip holds no second copy, that the Makefile rebuilds on a change
of the header, and the twiddle table's formula (host doubles rounded to float, the H-th roots and then the W-th) in numpy."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xmm-superres-denoise_amd", "csrc")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_one_copy_of_the_passes_in_the_header():
    hdr, fused = _read("sw_fft.h"), _read("swinfir.hip")
    for name in ("struct FftP", "float2 cmul(", "void fft_pass(", "void sw_fft_kernel(", "bool radices(", "struct FftShape", "hipError_t fft(",
                 "void fft_twiddles("):
        assert hdr.count(name) == 1, name
        assert name not in fused, name
    assert '#include "sw_fft.h"' in fused and "fft_twiddles(H, W, t.data())" in fused
    assert "#ifndef XSD_SW_FFT_H" in hdr and re.search(r"^namespace \{", hdr, re.M)
    # a kernel that allocates, waits or uses atomics would not fit an asynchronous caller
    assert "hipMalloc" not in hdr and "dev_alloc" not in hdr and "Synchronize" not in hdr and not re.search(r"atomic\w*\s*\(", hdr)


def test_the_makefile_rebuilds_on_a_change_of_the_header():
    mk = _read("Makefile")
    assert re.search(r"^HDRS :=.*\bsw_fft\.h\b", mk, re.M)


def test_the_twiddle_formula_is_the_roots_of_unity_in_double_rounded_to_float():
    """what fft_twiddles states, restated in numpy: exp(-2 pi i k / n) with cos and sin taken in double; cos(0) = 1 and sin(0) = -0.0 or
    0.0 exactly, and the quarter and half turns are exact to float rounding"""
    hdr = _read("sw_fft.h")
    assert "std::cos(-2.0 * pi * i / H)" in hdr and "std::sin(-2.0 * pi * i / H)" in hdr
    assert "std::cos(-2.0 * pi * i / W)" in hdr and "std::sin(-2.0 * pi * i / W)" in hdr and "t[H + i]" in hdr
    for n in (1, 3, 14, 22):
        a = -2.0 * np.pi * np.arange(n, dtype=np.float64) / n
        t = np.stack((np.cos(a), np.sin(a)), axis=1).astype(np.float32)
        assert t[0, 0] == 1.0 and t[0, 1] == 0.0
        assert np.allclose((t.astype(np.float64) ** 2).sum(1), 1.0, atol=2e-7)
        if n % 2 == 0:
            assert t[n // 2, 0] == -1.0 and abs(float(t[n // 2, 1])) < 1e-15
