"""Restormer without a GPU: the module's parameter names, shapes, order and default initialisation against the reference's
(tests/golden/restormer_keys_dim24.npz), the constructor refusals, the factory / config wiring, and the float64 restatement that is
the oracle of the GPU tests pinned to the reference's own float64 outputs (tests/golden/restormer_<case>.npz)."""
import json
import os

import numpy as np
import pytest
import torch

import gen_restormer as gr
import restormer_torch as rt

G = os.path.join(os.path.dirname(__file__), "golden")


def test_state_dict_names_shapes_order_and_init_match_reference():
    from xmm_superres_denoise.models import Restormer
    z = np.load(os.path.join(G, "restormer_keys_dim24.npz"))
    torch.manual_seed(0)
    sd = Restormer(1, 1, 24).state_dict()
    assert len(sd) == 494 and list(sd.keys()) == [str(n) for n in z["names"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(z["shapes"]))
    assert sum(v.numel() for v in sd.values()) == int(z["nparams"]) == 6674836
    # LayerNorm ones / zeros, temperature ones, torch's default conv init in the reference's construction order
    got = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    np.testing.assert_allclose(got, z["init_seed0"], rtol=1e-9, atol=1e-9)
    # the numpy helper that lays out the fixtures' weights agrees too
    assert list(gr.param_shapes(dict(inp_channels=1, out_channels=1, dim=24)).items()) == [(k, tuple(v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("case", list(gr.CASES))
def test_state_dict_layout_of_every_fixture_config(case):
    from xmm_superres_denoise.models import Restormer
    cfg = gr.CASES[case]["cfg"]
    sd = Restormer(**gr.full_cfg(**cfg)).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(gr.param_shapes(cfg).items())


def test_constructor_signature_and_refusals():
    import inspect
    from xmm_superres_denoise.models import Restormer
    sig = inspect.signature(Restormer.__init__)
    assert list(sig.parameters)[1:] == ["inp_channels", "out_channels", "dim", "num_blocks", "num_refinement_blocks", "heads",
                                        "ffn_expansion_factor", "bias", "LayerNorm_type", "dual_pixel_task"]
    assert sig.parameters["ffn_expansion_factor"].default == 2.66 and sig.parameters["LayerNorm_type"].default == "WithBias"
    with pytest.raises(ValueError, match="dual_pixel_task"):
        Restormer(6, 6, 24, dual_pixel_task=True)
    with pytest.raises(ValueError, match="inp_channels must equal out_channels"):
        Restormer(3, 1, 24)
    with pytest.raises(ValueError, match="even"):
        Restormer(1, 1, 25)
    with pytest.raises(ValueError, match="heads"):
        Restormer(1, 1, 24, heads=[5, 2, 4, 8])
    with pytest.raises(ValueError, match="channels per head"):
        Restormer(1, 1, 96, heads=[1, 2, 4, 8])        # 192 channels in one head at decoder level 1


def test_odd_ffn_hidden_widths_of_the_xmm_configuration():
    from xmm_superres_denoise.models import Restormer
    m = Restormer(1, 1, 24)
    hidden = [m.encoder_level1[0].ffn.project_out.in_channels, m.encoder_level2[0].ffn.project_out.in_channels,
              m.encoder_level3[0].ffn.project_out.in_channels, m.latent[0].ffn.project_out.in_channels]
    assert hidden == [63, 127, 255, 510]


def test_factory_and_config():
    from xmm_superres_denoise.config.config import MODELS_TOML, RestormerCfg, model_cfg
    from xmm_superres_denoise.models import Model, Restormer
    cfg = model_cfg("restormer", batch_size=2)
    assert isinstance(cfg.model, RestormerCfg) and cfg.model.dim == 24 and cfg.model.in_channels == cfg.model.out_channels == 1
    assert cfg.optimizer.learning_rate == 1e-4 and tuple(cfg.optimizer.betas) == (0.9, 0.999)
    assert MODELS_TOML["rrdb_denoise"]["filters"] == 32        # existing entries untouched
    m = Model(cfg, (416, 416), (416, 416))
    m.configure_model()
    assert isinstance(m.model, Restormer) and m.model.dim == 24 and m.model.num_blocks == [4, 6, 6, 8]


def test_training_restormer_is_refused_by_name():
    from xmm_superres_denoise.train import fit
    with pytest.raises(NotImplementedError, match="restormer"):
        fit("restormer", steps=1)


def test_forward_without_gpu_tensors_fails_loudly():
    from xmm_superres_denoise.models import Restormer
    with pytest.raises(RuntimeError):
        Restormer(1, 1, 8)(torch.zeros(1, 1, 16, 16))


@pytest.mark.parametrize("case", list(gr.CASES))
def test_float64_restatement_matches_reference_goldens(case):
    """the oracle of the GPU tests (restormer_torch.py, written for this project) against the reference's float64 output"""
    z = np.load(os.path.join(G, f"restormer_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    sd = {k: torch.from_numpy(v).double() for k, v in gr.make_state(cfg, int(z["seed"])).items()}
    x = gr.make_input(z["x"].shape, int(z["seed"]) + 1000)
    assert np.array_equal(x, z["x"])
    y = rt.restormer_forward(sd, torch.from_numpy(x).double(), **gr.full_cfg(**cfg)).numpy()
    assert np.abs(y - z["y64"]).max() < 1e-12
    # and the reference's fp32 output is a few ulps from it: the bar the engine is held to on the GPU
    assert np.abs(z["y32"] - z["y64"]).max() < 1e-5
