"""SwinIR without a GPU: the module's state-dict names, shapes, order, buffers and default initialisation against the reference's
(tests/golden/swinir_keys.npz, gen_swinir.param_shapes), the constructor's signature and refusals, the output-size rule and its C
binding, the header's declarations, and the float64-capable restatement (tests/golden/swinir_torch.py) that the GPU tests measure
against, pinned to the reference's own outputs (tests/golden/swinir_<case>.npz)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import gen_swinfir as gs
import gen_swinir as gi
import swinir_torch as si

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[1], num_heads=[2], window_size=4, upscale=1, upsampler="")


def _swinir(**cfg):
    from xmm_superres_denoise.models import SwinIR
    return SwinIR(**cfg)


def test_models_exports_swinir_with_the_reference_signature():
    import xmm_superres_denoise.models as M
    sig = inspect.signature(M.SwinIR.__init__)
    assert list(sig.parameters)[1:] == ["img_size", "patch_size", "in_chans", "embed_dim", "depths", "num_heads", "window_size",
                                        "mlp_ratio", "qkv_bias", "qk_scale", "drop_rate", "attn_drop_rate", "drop_path_rate", "norm_layer",
                                        "ape", "patch_norm", "use_checkpoint", "upscale", "img_range", "upsampler", "resi_connection"]
    for k, v in gi.DEFAULTS.items():
        assert sig.parameters[k].default == v, k
    assert sig.parameters["norm_layer"].default is torch.nn.LayerNorm


@pytest.mark.parametrize("case", list(gi.CASES))
def test_state_dict_layout_and_buffers_of_every_fixture_config(case):
    cfg = gi.CASES[case]["cfg"]
    sd = _swinir(**gi.full_cfg(**cfg)).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(gi.param_shapes(cfg).items())
    ws, shift, res = gi.window_of(cfg)
    nbuf = 0
    for k, v in sd.items():
        if k.endswith("relative_position_index"):
            assert np.array_equal(v.numpy(), gs.rel_index(ws)), k
            nbuf += 1
        elif k.endswith("attn_mask"):
            assert shift > 0 and np.array_equal(v.numpy(), gs.shift_mask(res[0], res[1], ws, shift)), k
            nbuf += 1
    assert nbuf == sum(cfg["depths"]) + (sum(d // 2 for d in cfg["depths"]) if shift else 0)


def test_state_dict_and_default_init_match_the_reference_under_one_seed():
    z = np.load(os.path.join(G, "swinir_keys.npz"))
    cfg = json.loads(str(z["cfg"]))
    assert cfg["embed_dim"] == 60 and cfg["upsampler"] == ""
    torch.manual_seed(0)
    m = _swinir(**gi.full_cfg(**cfg))
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in z["names"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(z["shapes"]))
    assert sum(p.numel() for p in m.parameters()) == int(z["nparams"])
    got = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    np.testing.assert_allclose(got, z["init_seed0"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("case", list(gi.CASES))
def test_restatement_matches_reference_goldens(case):
    """swinir_torch.py against the reference's own outputs: float64 to 1e-12 relative; in fp32 its error is within 2x of the
    reference's fp32 error (the bar the engine is held to on the GPU)"""
    z = np.load(os.path.join(G, f"swinir_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    assert cfg == gi.CASES[case]["cfg"] and tuple(z["x"].shape) == gi.CASES[case]["shape"]
    state = gi.make_state(cfg, int(z["seed"]))
    x = gi.make_input(z["x"].shape, int(z["seed"]) + 1000)
    assert np.array_equal(x, z["x"])
    sd64 = {k: torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(v) for k, v in state.items()}
    y = si.swinir_forward(sd64, torch.from_numpy(x).double(), **cfg).numpy()
    assert y.shape == z["y64"].shape
    assert np.abs(y - z["y64"]).max() <= 1e-12 * np.abs(z["y64"]).max()
    y32 = si.swinir_forward({k: torch.from_numpy(v) for k, v in state.items()}, torch.from_numpy(x), **cfg).numpy()

    def errs(a):
        e = np.abs(a.astype(np.float64) - z["y64"])
        return np.sqrt((e ** 2).mean()), e.max()

    (rms, mx), (rms_ref, mx_ref) = errs(y32), errs(z["y32"])
    print(f"{case}: restatement fp32 rms {rms:.3e} max {mx:.3e} | reference fp32 rms {rms_ref:.3e} max {mx_ref:.3e}")
    assert rms <= 2 * rms_ref and mx <= 2 * mx_ref
    up = cfg["upscale"]
    assert y.shape[2:] == (x.shape[2] * up, x.shape[3] * up)


def test_constructor_refusals_name_their_argument():
    from torch import nn
    _swinir(**OK)
    with pytest.raises(ValueError, match="ape=True"):
        _swinir(**dict(OK, ape=True))
    with pytest.raises(ValueError, match="upsampler"):
        _swinir(**dict(OK, upsampler="bicubic"))
    for rc in ("SFB", "identity"):
        with pytest.raises(ValueError, match="resi_connection"):
            _swinir(**dict(OK, resi_connection=rc))
    with pytest.raises(ValueError, match="norm_layer"):
        _swinir(**dict(OK, norm_layer=nn.BatchNorm1d))
    with pytest.raises(ValueError, match="num_heads"):
        _swinir(**dict(OK, num_heads=[3]))
    with pytest.raises(ValueError, match="head"):
        _swinir(**dict(OK, embed_dim=96, num_heads=[2]))                     # head dim 48 > 32
    with pytest.raises(ValueError, match="effective window"):
        _swinir(**dict(OK, img_size=64, window_size=24))
    with pytest.raises(ValueError, match="embed_dim"):
        _swinir(**dict(OK, embed_dim=2, num_heads=[1], resi_connection="3conv"))
    for up in (3, 8, 1):
        with pytest.raises(ValueError, match="nearest\\+conv.*upscale"):
            _swinir(**dict(OK, upsampler="nearest+conv", upscale=up))
    for up in (0, 5, 6, 16):
        with pytest.raises(ValueError, match=f"upscale {up}"):
            _swinir(**dict(OK, upscale=up))
    assert _swinir(**dict(OK, upsampler=None)).upsampler == ""                # the reference's docstring names None for denoising


def test_out_size_rule_and_binding():
    import ctypes
    from xmm_superres_denoise.engine import XsdError, _lib
    L = _lib.load()
    assert L.xsd_swinir_out_size.argtypes[1:3] == [ctypes.c_int, ctypes.c_int] and len(L.xsd_swinir_out_size.argtypes) == 5
    for s in ("create", "destroy", "param_count", "pack_weights", "forward", "out_size", "set_math", "get_math", "test_pad", "test_nearest_conv", "test_gemm_view"):
        assert "xsd_swinir_" + s in _lib.ABI_SYMBOLS and hasattr(L, "xsd_swinir_" + s)
    for case, spec in gi.CASES.items():
        m = _swinir(**gi.full_cfg(**spec["cfg"]))
        z = np.load(os.path.join(G, f"swinir_{case}.npz"))
        assert m.out_size(*spec["shape"][2:]) == tuple(z["y64"].shape[2:]), case
    m = _swinir(**dict(OK, window_size=8, img_size=32))
    assert m.out_size(9, 15) == (9, 15)                                       # pad 7 of 9: the largest legal pad
    with pytest.raises(XsdError, match="reflect pad"):
        m.out_size(4, 16)                                                     # pad 4 of 4
    with pytest.raises(XsdError, match="reflect pad"):
        m.out_size(16, 3)                                                     # pad 5 of 3
    g = _swinir(**dict(OK, img_size=20, patch_size=2, window_size=12))        # effective window 10, pads go to multiples of 12
    assert g.window == 10
    with pytest.raises(XsdError, match="window_size 12.*effective window 10"):
        g.out_size(24, 24)
    assert g.out_size(55, 60) == (55, 60)                                     # 60 is a multiple of both


def test_forward_without_gpu_tensors_fails_loudly():
    from xmm_superres_denoise.engine import XsdError
    m = _swinir(**OK)
    with pytest.raises(XsdError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 13, 16))
    with pytest.raises(XsdError, match="float32"):
        m(torch.zeros(1, 1, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match="f16x3"):
        m.set_math("f16x3")
    assert m.set_math("bf16x6").get_math() == "bf16x6"


def test_header_declares_the_swinir_entry_points():
    hdr = open(os.path.join(ROOT, "include", "xsd.h")).read()
    declared = set(re.findall(r"\b(xsd_swinir_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"xsd_swinir_" + s for s in ("create", "destroy", "param_count", "pack_weights", "forward", "out_size", "set_math",
                                                    "get_math", "test_pad", "test_nearest_conv", "test_gemm_view")}
    assert "typedef struct xsd_swinir_config" in hdr and "swinir.py:350-395" in hdr


def test_no_factory_entry_like_the_reference():
    from xmm_superres_denoise.config.config import MODELS_TOML
    assert not any("swinir" in k.lower() for k in MODELS_TOML)
