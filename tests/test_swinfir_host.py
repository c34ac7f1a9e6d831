"""SwinFIR without a GPU: the module's state-dict names, shapes, order and default initialisation against the reference's
(tests/golden/swinfir_keys_xmm.npz), the constructor refusals, the factory / config wiring, and the float64 restatement that is the
oracle of the GPU tests pinned to the reference's own float64 outputs (tests/golden/swinfir_<case>.npz)."""
import json
import os

import numpy as np
import pytest
import torch

import gen_swinfir as gs
import swinfir_torch as st

G = os.path.join(os.path.dirname(__file__), "golden")


def _xmm():
    from xmm_superres_denoise.models import SwinFIR
    return SwinFIR(**gs.full_cfg(**gs.XMM))


def test_state_dict_names_shapes_order_match_reference():
    z = np.load(os.path.join(G, "swinfir_keys_xmm.npz"))
    m = _xmm()
    sd = m.state_dict()
    assert len(sd) == 590 and list(sd.keys()) == [str(n) for n in z["names"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(z["shapes"]))
    assert sum(p.numel() for p in m.parameters()) == int(z["nparams"]) == 19045113
    assert list(gs.param_shapes(gs.XMM).items()) == [(k, tuple(v.shape)) for k, v in sd.items()]
    # the clamped window of the XMM configuration: 13 x 13 windows, no shift, no attn_mask buffer anywhere
    blk = m.layers[0].residual_group.blocks[1]
    assert blk.window_size == 13 and blk.shift_size == 0 and blk.attn_mask is None
    assert tuple(blk.attn.relative_position_bias_table.shape) == (625, 6)


def test_default_init_matches_reference_under_one_seed():
    z = np.load(os.path.join(G, "swinfir_keys_xmm.npz"))
    torch.manual_seed(0)
    sd = _xmm().state_dict()
    got = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    np.testing.assert_allclose(got, z["init_seed0"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("case", list(gs.CASES))
def test_state_dict_layout_and_buffers_of_every_fixture_config(case):
    from xmm_superres_denoise.models import SwinFIR
    cfg = gs.CASES[case]["cfg"]
    sd = SwinFIR(**gs.full_cfg(**cfg)).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(gs.param_shapes(cfg).items())
    ref = gs.make_state(cfg, 1)
    for k, v in sd.items():
        if k.endswith("relative_position_index") or k.endswith("attn_mask"):
            assert np.array_equal(v.numpy(), ref[k]), k


def test_model_cfg_builds_the_xmm_configuration():
    from xmm_superres_denoise.config.config import MODELS_TOML, TransformerCfg, model_cfg
    from xmm_superres_denoise.models import Model, SwinFIR
    cfg = model_cfg("swinfir")
    assert isinstance(cfg.model, TransformerCfg) and cfg.model.embed_dim == 180 and cfg.model.patch_size == 32
    assert cfg.model.depths == [6] * 6 and cfg.model.num_heads == [6] * 6 and cfg.model.upsampler == "pixelshuffle"
    assert cfg.optimizer.learning_rate == 2e-4
    assert MODELS_TOML["restormer"]["dim"] == 24               # existing entries untouched
    m = Model(cfg, (416, 416), (832, 832))
    m.configure_model()
    assert isinstance(m.model, SwinFIR) and m.model.upscale == 2 and m.model.resi_connection == "SFB" and m.model.window == 13
    assert [k for k in m.model.state_dict()] == [str(n) for n in np.load(os.path.join(G, "swinfir_keys_xmm.npz"))["names"]]


def test_drct_and_hat_stay_refused_by_name():
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.models import Model
    with pytest.raises(NotImplementedError, match="drct: .*dead code"):
        Model(model_cfg("drct"), (416, 416), (832, 832)).configure_model()
    with pytest.raises(NotImplementedError, match="HAT"):
        Model(model_cfg("hat"), (416, 416), (832, 832)).configure_model()


def test_constructor_refusals():
    import inspect
    from torch import nn
    from xmm_superres_denoise.models import SwinFIR
    sig = inspect.signature(SwinFIR.__init__)
    assert list(sig.parameters)[1:] == ["img_size", "patch_size", "in_chans", "embed_dim", "depths", "num_heads", "window_size",
                                        "mlp_ratio", "qkv_bias", "qk_scale", "drop_rate", "attn_drop_rate", "drop_path_rate", "norm_layer",
                                        "ape", "patch_norm", "use_checkpoint", "upscale", "img_range", "upsampler", "resi_connection"]
    ok = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[1], num_heads=[2], window_size=4, upsampler="pixelshuffle")
    SwinFIR(**ok)
    with pytest.raises(ValueError, match="ape=True"):
        SwinFIR(**dict(ok, ape=True))
    for u in ("", "pixelshuffledirect", "nearest+conv"):
        with pytest.raises(ValueError, match="upsampler"):
            SwinFIR(**dict(ok, upsampler=u))
    for rc in ("HSFB", "identity", "3conv"):
        with pytest.raises(ValueError, match="resi_connection"):
            SwinFIR(**dict(ok, resi_connection=rc))
    with pytest.raises(ValueError, match="norm_layer"):
        SwinFIR(**dict(ok, norm_layer=nn.BatchNorm1d))
    with pytest.raises(ValueError, match="num_heads"):
        SwinFIR(**dict(ok, num_heads=[3]))
    with pytest.raises(ValueError, match="at most 32 channels per head"):
        SwinFIR(**dict(ok, embed_dim=96, num_heads=[2]))
    with pytest.raises(ValueError, match="effective window"):
        SwinFIR(**dict(ok, img_size=64, window_size=24))
    with pytest.raises(ValueError, match="scale 5"):
        SwinFIR(**dict(ok, upscale=5))


def test_training_swinfir_is_refused_by_name():
    from xmm_superres_denoise.train import fit
    with pytest.raises(NotImplementedError, match="swinfir"):
        fit("swinfir", steps=1)


def test_forward_without_gpu_tensors_fails_loudly():
    from xmm_superres_denoise.models import SwinFIR
    m = SwinFIR(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[1], num_heads=[2], window_size=4, upsampler="pixelshuffle")
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 16, 16))


@pytest.mark.parametrize("case", list(gs.CASES))
def test_float64_restatement_matches_reference_goldens(case):
    """the oracle of the GPU tests (swinfir_torch.py, written for this project) against the reference's float64 output"""
    z = np.load(os.path.join(G, f"swinfir_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    sd = {k: torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(v) for k, v in
          gs.make_state(cfg, int(z["seed"])).items()}
    x = gs.make_input(z["x"].shape, int(z["seed"]) + 1000)
    assert np.array_equal(x, z["x"])
    y = st.swinfir_forward(sd, torch.from_numpy(x).double(), **cfg).numpy()
    assert y.shape == z["y64"].shape
    assert np.abs(y - z["y64"]).max() < 1e-12
    # and the reference's fp32 output is a few ulps from it: the bar the engine is held to on the GPU
    assert np.abs(z["y32"] - z["y64"]).max() < 1e-5
