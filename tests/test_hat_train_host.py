"""What the trainable HAT promises without a device: the ABI of the two differentiable HAT ops (header <-> _lib.ENTRIES <-> both
libraries), their scratch queries and the refusals the library answers before it touches a device, the wrapper's shared Parameter
objects and reference key names, and the refusals that need no GPU."""
import copy
import ctypes
import os
import re

import pytest
import torch

import gen_hat as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["xsd_hat_op_ocab_forward", "xsd_hat_op_ocab_scratch", "xsd_hat_op_ocab_backward", "xsd_hat_op_ca_forward", "xsd_hat_op_ca_scratch",
       "xsd_hat_op_ca_backward"]
TINY = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=4, overlap_ratio=0.5,
            compress_ratio=3, squeeze_factor=4, mlp_ratio=2.0, upscale=2, upsampler="pixelshuffle", resi_connection="1conv")


def _al(n):
    return n + (-n % 256)


def test_header_entries_and_both_libraries_agree_on_the_ops():
    from test_abi import exported_xsd_symbols
    from xmm_superres_denoise.engine import _lib
    hdr = open(os.path.join(ROOT, "include", "xsd.h")).read()
    assert sorted(set(re.findall(r"\b(xsd_hat_op_\w+)\s*\(", hdr))) == sorted(OPS)
    assert [n for n in _lib.ENTRIES if n.startswith("xsd_hat_op_")] == OPS                       # the header's order
    hooks = os.path.join(os.path.dirname(_lib.LIB_PATH), "libxsd_hip_hooks.so")
    for lib in (_lib.LIB_PATH, hooks):
        assert set(OPS) <= exported_xsd_symbols(lib), lib
    p, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert _lib.ENTRIES["xsd_hat_op_ocab_forward"] == (i, [p, p, p, i, i, i, i, i, i, i, f, p])
    assert _lib.ENTRIES["xsd_hat_op_ocab_scratch"] == (i64, [i] * 7)
    assert _lib.ENTRIES["xsd_hat_op_ocab_backward"] == (i, [p] * 6 + [i] * 7 + [f, p, i64, p])
    assert _lib.ENTRIES["xsd_hat_op_ca_forward"] == (i, [p] * 7 + [i, i64, i, i, p, i64, p])
    assert _lib.ENTRIES["xsd_hat_op_ca_scratch"] == (i64, [i, i64, i, i, i])
    assert _lib.ENTRIES["xsd_hat_op_ca_backward"] == (i, [p] * 11 + [i, i64, i, i, p, i64, p])
    csrc = os.path.join(ROOT, "xmm-superres-denoise_amd", "csrc")
    src = open(os.path.join(csrc, "hat_ops.hip")).read()
    assert "hipMalloc" not in src and "dev_alloc" not in src and "Synchronize" not in src and not re.search(r"atomic\w*\s*\(", src)   # allocates nothing, never waits, no atomics
    assert "hat_ops.hip" in open(os.path.join(csrc, "Makefile")).read()
    # the shared kernels live in one header that both translation units include
    for name in ("hat.hip", "hat_ops.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "hat_kernels.h"' in text and "void hat_ocab_kernel" not in text and "void hat_ca_kernel" not in text, name


def test_scratch_queries_return_the_documented_bytes_and_refuse_by_name():
    from xmm_superres_denoise.engine import _lib
    L = _lib.load()
    # overlap_attention: 4 nwin ow^2 2 C + 4 nwin (ws + ow - 1)^2 heads, each term rounded up to 256
    assert L.xsd_hat_op_ocab_scratch(2, 8, 12, 12, 2, 4, 6) == _al(4 * 12 * 36 * 24) + _al(4 * 12 * 81 * 2)
    assert L.xsd_hat_op_ocab_scratch(1, 32, 48, 60, 2, 16, 24) == _al(4 * 6 * 576 * 120) + _al(4 * 6 * 39 * 39 * 2)
    # channel_attention: forward 8 B chunks C + 4 B C; backward 8 B chunks 2 C + 8 B (3 C + Cs) + 8 B (2 Cs C + Cs + C)
    assert L.xsd_hat_op_ca_scratch(3, 257, 180, 6, 0) == _al(8 * 3 * 2 * 180) + _al(4 * 3 * 180)
    assert L.xsd_hat_op_ca_scratch(3, 257, 180, 6, 1) == _al(8 * 3 * 2 * 360) + _al(8 * 3 * (3 * 180 + 6)) + _al(8 * 3 * (2 * 6 * 180 + 6 + 180))
    assert L.xsd_hat_op_ca_scratch(2, 96, 12, 3, 0) == _al(8 * 2 * 12) + _al(4 * 2 * 12)
    assert L.xsd_hat_op_ca_scratch(2, 96, 12, 3, 1) == _al(8 * 2 * 24) + _al(8 * 2 * (3 * 12 + 3)) + _al(8 * 2 * (2 * 3 * 12 + 3 + 12))
    for call, msg in ((lambda: L.xsd_hat_op_ocab_scratch(1, 17, 17, 8, 2, 17, 19), b"overlap_attention: window size 17 is outside [1, 16]"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 16, 16, 8, 2, 16, 34), b"overlap_attention: overlap window 34 is outside [window size 16, 32]"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 8, 8, 8, 2, 4, 3), b"overlap_attention: overlap window 3 is outside [window size 4, 32]"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 8, 8, 8, 2, 4, 7), b"overlap_attention: overlap window 7 minus window size 4 is odd"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 8, 8, 66, 2, 4, 6), b"overlap_attention: head dim 33; the kernel takes at most 32"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 8, 10, 8, 2, 4, 6), b"overlap_attention: H and W must be multiples of the window size 4; got 8 x 10"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 8, 8, 9, 2, 4, 6), b"overlap_attention: 2 heads do not divide 9 channels"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 2, 2, 4, 2, 1, 1), b"overlap_attention: window size 1 with an overlap window of 1 indexes past"),
                      (lambda: L.xsd_hat_op_ocab_scratch(1, 16384, 16384, 1024, 32, 16, 16), b"overlap_attention: 1 x 16384 x 16384 tokens of 1024 channels are too many elements"),
                      (lambda: L.xsd_hat_op_ca_scratch(65536, 4, 4, 2, 0), b"channel_attention: 65536 images are outside [1, 65535]"),
                      (lambda: L.xsd_hat_op_ca_scratch(1, (1 << 28) + 1, 4, 2, 1), b"channel_attention: 268435457 pixels are outside [1, 2^28]"),
                      (lambda: L.xsd_hat_op_ca_scratch(1, 4, 4097, 2, 1), b"channel_attention: 4097 channels are outside [1, 4096]"),
                      (lambda: L.xsd_hat_op_ca_scratch(1, 4, 4, 0, 0), b"channel_attention: a squeezed width of 0 is outside [1, 4096]")):
        assert call() == -1 and msg in L.xsd_last_error(), (msg, L.xsd_last_error())


def test_entries_answer_null_pointers_before_touching_a_device():
    from xmm_superres_denoise.engine import _lib
    L = _lib.load()
    err = L.xsd_last_error
    assert L.xsd_hat_op_ocab_forward(None, None, None, 1, 8, 8, 8, 2, 4, 6, 1.0, None) != 0 and b"overlap_attention: null argument" in err()
    assert L.xsd_hat_op_ocab_backward(None, None, None, None, None, None, 1, 8, 8, 8, 2, 4, 6, 1.0, None, 0, None) != 0
    assert b"overlap_attention: null argument" in err()
    assert L.xsd_hat_op_ca_forward(None, None, None, None, None, None, None, 1, 4, 4, 2, None, 0, None) != 0
    assert b"channel_attention: null argument" in err()
    assert L.xsd_hat_op_ca_backward(*([None] * 11), 1, 4, 4, 2, None, 0, None) != 0 and b"channel_attention: null argument" in err()


def test_ops_refuse_cpu_tensors_by_name():
    from xmm_superres_denoise import ops
    from xmm_superres_denoise.engine import XsdError
    assert {"overlap_attention", "channel_attention"} <= set(ops.__all__)
    z = torch.zeros
    with pytest.raises(XsdError, match="qkv must be a CUDA.*no CPU fallback"):
        ops.overlap_attention(z(1, 64, 24), z(81, 2), 8, 8, 2, 4, 6, 1.0)
    with pytest.raises(XsdError, match="t must be a CUDA.*no CPU fallback"):
        ops.channel_attention(z(1, 16, 8), z(2, 8, 1, 1), z(2), z(8, 2, 1, 1), z(8))


def test_wrapper_shares_the_parameters_and_keeps_the_reference_names():
    from xmm_superres_denoise.models import HAT, SwinFIR, TrainableHAT
    m = HAT(**TINY)
    net = TrainableHAT(m)
    assert [id(p) for p in net.parameters()] == [id(p) for p in m.parameters()]
    assert list(net.state_dict()) == list(m.state_dict()) == list(gh.param_shapes(TINY))
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v for k, v in m.state_dict().items()}
    net.load_state_dict(sd)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    assert [id(p) for p in net.parameters()] == [id(p) for p in m.parameters()]
    other = copy.deepcopy(net)
    assert other.module is not m and list(other.state_dict()) == list(m.state_dict())
    assert m.drop_path_rate == 0.1 and net.drop_path_rate == 0.1 and TrainableHAT(m, drop_path_rate=0.0).drop_path == [0.0] * 4
    assert TrainableHAT(HAT(**dict(TINY, resi_connection="identity"))).module.resi_connection == "identity"
    with pytest.raises(Exception, match="no CPU fallback"):
        net(torch.zeros(1, 1, 8, 8))
    with pytest.raises(TypeError, match=r"TrainableHAT wraps a models.HAT \(got Linear\)"):
        TrainableHAT(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match=r"TrainableHAT wraps a models.HAT \(got SwinFIR\)"):
        TrainableHAT(SwinFIR(img_size=16, patch_size=1, in_chans=1, embed_dim=12, depths=[2], num_heads=[2], window_size=4, upscale=2,
                             upsampler="pixelshuffle", resi_connection="1conv"))
    with pytest.raises(NotImplementedError, match="TrainableHAT: drop_rate = 0.1 is not supported"):
        TrainableHAT(HAT(**dict(TINY, drop_rate=0.1)))
    with pytest.raises(NotImplementedError, match="TrainableHAT: attn_drop_rate = 0.2 is not supported"):
        TrainableHAT(HAT(**dict(TINY, attn_drop_rate=0.2)))
    with pytest.raises(ValueError, match=r"drop_path_rate 1.0 is outside \[0, 1\)"):
        TrainableHAT(m, drop_path_rate=1.0)


def test_fit_still_refuses_hat_and_fit_hat_fails_loudly_without_a_device():
    from xmm_superres_denoise import train
    with pytest.raises(NotImplementedError, match="hat: training"):
        train.fit("hat")
    with pytest.raises(ValueError, match="fit_hat: loss 'mse' is not supported") if torch.cuda.is_available() else \
            pytest.raises(RuntimeError, match="no HIP device visible"):
        train.fit_hat(TINY, loss="mse")
