"""What the trainable SwinIR promises without a device: the ABI of the differentiable ops (header <-> _lib.ABI_SYMBOLS <-> library), the
wrapper's shared Parameter objects and reference key names, the refusals that need no GPU, and the DropPath schedule."""
import copy
import os
import re

import pytest
import torch

import gen_swinir as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["xsd_sw_op_linear_scratch", "xsd_sw_op_linear_forward", "xsd_sw_op_linear_backward", "xsd_sw_op_conv3x3_scratch",
       "xsd_sw_op_conv3x3_forward", "xsd_sw_op_conv3x3_backward", "xsd_sw_op_layernorm_forward", "xsd_sw_op_layernorm_scratch",
       "xsd_sw_op_layernorm_backward", "xsd_sw_op_attention_forward", "xsd_sw_op_attention_scratch", "xsd_sw_op_attention_backward"]
TINY = dict(img_size=64, in_chans=1, embed_dim=12, depths=[2, 3], num_heads=[2, 2], window_size=4, upscale=1, upsampler="")


def test_header_abi_symbols_and_library_agree_on_the_ops():
    import ctypes
    from xmm_superres_denoise.engine import _lib
    hdr = open(os.path.join(ROOT, "include", "xsd.h")).read()
    declared = set(re.findall(r"\b(xsd_sw_op_\w+)\s*\(", hdr))
    assert declared == set(OPS) and set(OPS) <= set(_lib.ABI_SYMBOLS)
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(L, s) for s in OPS)
    src = open(os.path.join(ROOT, "xmm-superres-denoise_amd", "csrc", "sw_ops.hip")).read()
    assert "hipMalloc" not in src and "dev_alloc" not in src and "Synchronize" not in src and not re.search(r"atomic\w*\s*\(", src)   # allocates nothing, never waits, no atomics
    assert "sw_ops.hip" in open(os.path.join(ROOT, "xmm-superres-denoise_amd", "csrc", "Makefile")).read()


def test_scratch_queries_and_refusals_of_the_library_need_no_device():
    from xmm_superres_denoise.engine import _lib
    L = _lib.load()
    assert L.xsd_sw_op_linear_scratch(480, 36, 70, 0, 0, 0) == 36 * 70 * 4 + (-(36 * 70 * 4) % 256)
    one = L.xsd_sw_op_linear_scratch(480, 36, 70, 0, 480, 1)
    five = L.xsd_sw_op_linear_scratch(480, 36, 70, 0, 112, 1)          # 5 partials of 70 x 37
    assert one == 70 * 37 * 4 + (-(70 * 37 * 4) % 256) and five == 5 * 70 * 37 * 4 + (-(5 * 70 * 37 * 4) % 256)
    assert L.xsd_sw_op_linear_scratch(480, 36, 70, 1, 480, 1) == one + 480 * 70 * 4          # the activation's dz
    assert L.xsd_sw_op_attention_scratch(2, 16, 24, 16, 2, 8) == 2 * 6 * 225 * 2 * 4 + (-(2 * 6 * 225 * 2 * 4) % 256)
    assert L.xsd_sw_op_layernorm_scratch(300, 24) == 300 * 16 + (-(300 * 16) % 256) + 3 * 2 * 24 * 4 + (-(3 * 2 * 24 * 4) % 256)
    for call, msg in ((lambda: L.xsd_sw_op_linear_scratch(0, 8, 8, 0, 0, 0), b"linear: 0 rows are outside [1, 2^28]"),
                      (lambda: L.xsd_sw_op_linear_scratch(5000, 8, 8, 0, 1, 1), b"into 5000 partials; at most 4096"),
                      (lambda: L.xsd_sw_op_conv3x3_scratch(1, 4, 4, 2, 6, 5, 0, 0), b"conv3x3: activation 5"),
                      (lambda: L.xsd_sw_op_layernorm_scratch(4, 4097), b"layer_norm: 4097 channels are outside [1, 4096]"),
                      (lambda: L.xsd_sw_op_attention_scratch(1, 17, 17, 8, 2, 17), b"window_attention: window size 17 is outside [1, 16]"),
                      (lambda: L.xsd_sw_op_attention_scratch(1, 8, 8, 66, 2, 4), b"window_attention: head dim 33; the kernel takes at most 32")):
        assert call() == -1 and msg in L.xsd_last_error(), msg
    # null pointers and a refused math mode are answered before anything touches a device
    assert L.xsd_sw_op_linear_forward(None, None, None, None, None, 4, 8, 6, 0, 0.01, 3, None, 0, None) != 0
    assert b"linear: math mode bf16x6 is not supported by the differentiable ops (fp32 only)" in L.xsd_last_error()
    assert L.xsd_sw_op_layernorm_forward(None, None, None, None, 4, 8, None) != 0 and b"layer_norm: null argument" in L.xsd_last_error()


def test_ops_refuse_cpu_tensors_and_bf16x6_by_name():
    from xmm_superres_denoise import ops
    from xmm_superres_denoise.engine import XsdError
    z = torch.zeros
    with pytest.raises(XsdError, match="no CPU fallback"):
        ops.linear(z(4, 8), z(6, 8))
    with pytest.raises(XsdError, match="no CPU fallback"):
        ops.window_attention(z(1, 16, 24), z(49, 2), 4, 4, 2, 4, 0, 1.0)
    with pytest.raises(XsdError, match="math mode 'bf16x6' is not supported by the differentiable ops"):
        ops.conv3x3(z(1, 4, 4, 2), z(6, 2, 3, 3), math="bf16x6")
    with pytest.raises(XsdError, match="unknown activation 'silu'"):
        ops.linear(z(4, 8), z(6, 8), act="silu")


def test_wrapper_shares_the_parameters_and_keeps_the_reference_names():
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    m = SwinIR(**TINY)
    net = TrainableSwinIR(m)
    assert [id(p) for p in net.parameters()] == [id(p) for p in m.parameters()]
    assert list(net.state_dict()) == list(m.state_dict()) == list(gi.param_shapes(TINY))
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v for k, v in m.state_dict().items()}
    net.load_state_dict(sd)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    assert [id(p) for p in net.parameters()] == [id(p) for p in m.parameters()]
    other = copy.deepcopy(net)
    assert other.module is not m and list(other.state_dict()) == list(m.state_dict())
    assert m.drop_path_rate == 0.1 and net.drop_path_rate == 0.1 and TrainableSwinIR(m, drop_path_rate=0.0).drop_path == [0.0] * 5
    with pytest.raises(Exception, match="no CPU fallback"):
        net(torch.zeros(1, 1, 8, 8))
    with pytest.raises(TypeError, match="wraps a models.SwinIR"):
        TrainableSwinIR(torch.nn.Linear(2, 2))


@pytest.mark.parametrize("kw,msg", [
    (dict(upsampler="pixelshuffledirect", upscale=2), "upsampler 'pixelshuffledirect' is not trainable"),
    (dict(upsampler="nearest+conv", upscale=2), r"upsampler 'nearest\+conv' is not trainable"),
    (dict(resi_connection="3conv"), r"resi_connection '3conv' \(\"3conv\"\) is not trainable"),
    (dict(drop_rate=0.1), "drop_rate = 0.1 is not supported"),
    (dict(attn_drop_rate=0.2), "attn_drop_rate = 0.2 is not supported"),
])
def test_constructor_refusals_by_name(kw, msg):
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    with pytest.raises(NotImplementedError, match=msg):
        TrainableSwinIR(SwinIR(**dict(TINY, **kw)))


def test_drop_path_schedule_is_the_references_linspace():
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    from xmm_superres_denoise.models.modules.swinir_train import drop_path_schedule
    assert drop_path_schedule([2, 3], 0.1) == [x.item() for x in torch.linspace(0, 0.1, 5)]
    assert drop_path_schedule([6] * 6, 0.1)[0] == 0.0 and abs(drop_path_schedule([6] * 6, 0.1)[-1] - 0.1) < 1e-8
    net = TrainableSwinIR(SwinIR(**TINY), drop_path_rate=0.3)
    assert net.drop_path == drop_path_schedule([2, 3], 0.3) and len(net.drop_path) == 5
    with pytest.raises(ValueError, match=r"drop_path_rate 1.0 is outside \[0, 1\)"):
        TrainableSwinIR(SwinIR(**TINY), drop_path_rate=1.0)


def test_fit_is_untouched_and_fit_swinir_fails_loudly_without_a_device():
    from xmm_superres_denoise import train
    for name in ("restormer", "swinfir", "hat"):
        with pytest.raises(NotImplementedError, match=f"{name}: training"):
            train.fit(name)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            train.fit_swinir(TINY)
