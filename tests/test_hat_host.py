"""HAT without a GPU: the module's constructor signature, state-dict names, shapes, order and default initialisation against the
reference's (tests/golden/hat_keys_xmm.npz), every constructor refusal by message, the factory / config wiring (refused without the
forward_only_hat keyword, built with it), and the float64 restatement that is the oracle of the GPU tests pinned to the reference's own
float64 outputs (tests/golden/hat_<case>.npz)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import gen_hat as gh
import hat_torch as ht

G = os.path.join(os.path.dirname(__file__), "golden")


def _xmm():
    from xmm_superres_denoise.models import HAT
    return HAT(**gh.full_cfg(**gh.XMM))


def test_constructor_signature_and_defaults_match_reference():
    from torch import nn
    from xmm_superres_denoise.models import HAT
    sig = inspect.signature(HAT.__init__)
    assert list(sig.parameters)[1:] == ["img_size", "patch_size", "in_chans", "embed_dim", "depths", "num_heads", "window_size",
                                        "compress_ratio", "squeeze_factor", "conv_scale", "overlap_ratio", "mlp_ratio", "qkv_bias",
                                        "qk_scale", "drop_rate", "attn_drop_rate", "drop_path_rate", "norm_layer", "ape", "patch_norm",
                                        "use_checkpoint", "upscale", "img_range", "upsampler", "resi_connection"]
    got = {k: (list(v.default) if isinstance(v.default, tuple) else v.default) for k, v in list(sig.parameters.items())[1:]}
    assert got.pop("norm_layer") is nn.LayerNorm
    assert got == gh.DEFAULTS


def test_state_dict_names_shapes_order_match_reference():
    z = np.load(os.path.join(G, "hat_keys_xmm.npz"))
    m = _xmm()
    sd = m.state_dict()
    assert len(sd) == 862 and list(sd.keys()) == [str(n) for n in z["names"]]
    assert list(sd.keys())[:2] == ["relative_position_index_SA", "relative_position_index_OCA"]
    assert not any("attn_mask" in k for k in sd)
    assert [list(v.shape) for v in sd.values()] == json.loads(str(z["shapes"]))
    assert sum(p.numel() for p in m.parameters()) == int(z["nparams"]) == 26078721
    assert list(gh.param_shapes(gh.XMM).items()) == [(k, tuple(v.shape)) for k, v in sd.items()]
    # the XMM configuration: 26 x 26 patches > the 16 x 16 window, so odd blocks shift by 8; 24 x 24 keys per overlapping window
    blk = m.layers[0].residual_group.blocks[1]
    assert blk.window_size == 16 and blk.shift_size == 8
    assert tuple(m.layers[0].residual_group.overlap_attn.relative_position_bias_table.shape) == (39 * 39, 6)
    assert tuple(m.relative_position_index_OCA.shape) == (256, 576) and int(m.relative_position_index_OCA.min()) < 0


def test_default_init_matches_reference_under_one_seed():
    z = np.load(os.path.join(G, "hat_keys_xmm.npz"))
    torch.manual_seed(0)
    sd = _xmm().state_dict()
    got = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    np.testing.assert_allclose(got, z["init_seed0"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("case", list(gh.CASES))
def test_state_dict_layout_and_buffers_of_every_fixture_config(case):
    from xmm_superres_denoise.models import HAT
    cfg = gh.CASES[case]["cfg"]
    sd = HAT(**gh.full_cfg(**cfg)).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(gh.param_shapes(cfg).items())
    ref = gh.make_state(cfg, 1)
    for k, v in sd.items():
        if k.startswith("relative_position_index"):
            assert np.array_equal(v.numpy(), ref[k]), k


def test_constructor_refusals():
    from torch import nn
    from xmm_superres_denoise.models import HAT
    ok = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[1], num_heads=[2], window_size=4, squeeze_factor=4,
              upsampler="pixelshuffle")
    HAT(**ok)
    HAT(**dict(ok, img_size=4))                       # img_size // patch_size == window_size: fine, no block shifts
    HAT(**dict(ok, qk_scale=0))                       # 0 and None: head_dim^-0.5
    with pytest.raises(ValueError, match="ape=True"):
        HAT(**dict(ok, ape=True))
    for u in ("", "pixelshuffledirect", "nearest+conv"):
        with pytest.raises(ValueError, match="upsampler"):
            HAT(**dict(ok, upsampler=u))
    for rc in ("SFB", "3conv"):
        with pytest.raises(ValueError, match="resi_connection"):
            HAT(**dict(ok, resi_connection=rc))
    with pytest.raises(ValueError, match="norm_layer"):
        HAT(**dict(ok, norm_layer=nn.BatchNorm1d))
    with pytest.raises(ValueError, match="does not divide embed_dim"):
        HAT(**dict(ok, num_heads=[3]))
    with pytest.raises(ValueError, match="at most 32 channels per head"):
        HAT(**dict(ok, embed_dim=96, num_heads=[2]))
    with pytest.raises(ValueError, match="window_size 24 is not supported"):
        HAT(**dict(ok, img_size=64, window_size=24))
    with pytest.raises(ValueError, match="overlap window of 36 is not supported"):
        HAT(**dict(ok, img_size=16, window_size=12, overlap_ratio=2.0))
    with pytest.raises(ValueError, match=r"int\(window_size \* overlap_ratio\) = 3 is odd"):
        HAT(**dict(ok, img_size=12, window_size=6, overlap_ratio=0.5))
    with pytest.raises(ValueError, match="squeeze_factor"):
        HAT(**dict(ok, squeeze_factor=30))            # 16 // 30 == 0 (the class default on a narrow model)
    with pytest.raises(ValueError, match="compress_ratio"):
        HAT(**dict(ok, compress_ratio=17))
    with pytest.raises(ValueError, match="smaller than window_size 4"):
        HAT(**dict(ok, img_size=3))
    with pytest.raises(ValueError, match="qk_scale"):
        HAT(**dict(ok, qk_scale=-0.1))


def test_factory_refuses_hat_without_the_keyword_and_builds_it_with_it():
    from xmm_superres_denoise.config.config import TransformerCfg, model_cfg
    from xmm_superres_denoise.models import HAT, Model
    cfg = model_cfg("hat")
    assert isinstance(cfg.model, TransformerCfg) and cfg.model.embed_dim == 180 and cfg.model.patch_size == 16
    with pytest.raises(NotImplementedError, match="HAT is forward-only.*models.HAT.*infer.load_model.*train test"):
        Model(cfg, (416, 416), (832, 832)).configure_model()
    m = Model(cfg, (416, 416), (832, 832))
    m.configure_model(forward_only_hat=True)
    assert isinstance(m.model, HAT) and m.model.upscale == 2 and m.model.resi_connection == "1conv" and m.model.window == 16
    assert [k for k in m.model.state_dict()] == [str(n) for n in np.load(os.path.join(G, "hat_keys_xmm.npz"))["names"]]
    # the keyword opens nothing else
    with pytest.raises(NotImplementedError, match="drct"):
        Model(model_cfg("drct"), (416, 416), (832, 832)).configure_model(forward_only_hat=True)


def test_training_hat_is_refused_by_name():
    from xmm_superres_denoise.train import fit
    with pytest.raises(NotImplementedError, match="hat: training HAT is not on the MI355X engine"):
        fit("hat", steps=1)


def test_forward_without_gpu_tensors_fails_loudly():
    from xmm_superres_denoise.models import HAT
    m = HAT(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[1], num_heads=[2], window_size=4, squeeze_factor=4,
            upsampler="pixelshuffle")
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 16, 16))


@pytest.mark.parametrize("case", list(gh.CASES))
def test_float64_restatement_matches_reference_goldens(case):
    """the oracle of the GPU tests (hat_torch.py, written for this project) against the reference's float64 output"""
    z = np.load(os.path.join(G, f"hat_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    assert cfg == gh.CASES[case]["cfg"]
    sd = {k: torch.from_numpy(v).double() if v.dtype == np.float32 else torch.from_numpy(v) for k, v in
          gh.make_state(cfg, int(z["seed"])).items()}
    x = gh.make_input(z["x"].shape, int(z["seed"]) + 1000)
    assert np.array_equal(x, z["x"])
    y = ht.hat_forward(sd, torch.from_numpy(x).double(), **cfg).numpy()
    assert y.shape == z["y64"].shape
    assert np.abs(y - z["y64"]).max() < 1e-12
    # and the reference's fp32 output is a few ulps from it: the bar the engine is held to on the GPU
    assert np.abs(z["y32"] - z["y64"]).max() < 1e-5
