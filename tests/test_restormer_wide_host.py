"""Restormer past 64 channels per head, without a GPU: the published network `Restormer()` (dim 48: decoder_level1 and the refinement run
96 channels on one head) constructs with the reference's parameter names, shapes, order and default initialisation
(tests/golden/restormer_keys_dim48.npz); the limit is 128 channels per head; the float64 restatement reproduces the reference's float64
output of the two wide fixtures (tests/golden/gen_restormer_wide.py); `dim` reaches the factory through infer.load_model / train.test /
`train test --dim` and is refused by name with any other model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import gen_restormer_wide as gw
import restormer_torch as rt

G = os.path.join(os.path.dirname(__file__), "golden")


def test_published_defaults_construct_and_match_the_reference_state_dict():
    from xmm_superres_denoise.models import Restormer
    z = np.load(os.path.join(G, "restormer_keys_dim48.npz"))
    torch.manual_seed(0)
    m = Restormer()
    assert (m.dim, m.inp_channels, m.out_channels, m.heads, m.num_blocks) == (48, 3, 3, [1, 2, 4, 8], [4, 6, 6, 8])
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in z["names"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(z["shapes"]))
    assert sum(v.numel() for v in sd.values()) == int(z["nparams"]) == 26126644
    got = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    np.testing.assert_allclose(got, z["init_seed0"], rtol=1e-9, atol=1e-9)
    assert list(gw.param_shapes({}).items()) == [(k, tuple(v.shape)) for k, v in sd.items()]


def test_the_limit_is_128_channels_per_head():
    from xmm_superres_denoise.models import Restormer
    from xmm_superres_denoise.models.modules.restormer import MAX_CHANNELS_PER_HEAD
    assert MAX_CHANNELS_PER_HEAD == 128
    m = Restormer(1, 1, 64)                                # 128 channels on one head at decoder level 1
    assert m.decoder_level1[0].attn.qkv.in_channels == 128 and m.decoder_level1[0].attn.num_heads == 1
    with pytest.raises(ValueError, match=r"heads\[0\] = 1 must divide the 132 channels of its level into at most 128 channels per head"):
        Restormer(1, 1, 66)
    with pytest.raises(ValueError, match="channels per head"):
        Restormer(1, 1, 96)                                # 192: refused as before


@pytest.mark.parametrize("case", list(gw.CASES))
def test_state_dict_layout_of_the_wide_fixture_configs(case):
    from xmm_superres_denoise.models import Restormer
    cfg = gw.CASES[case]["cfg"]
    sd = Restormer(**gw.full_cfg(**cfg)).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(gw.param_shapes(cfg).items())


@pytest.mark.parametrize("case", list(gw.CASES))
def test_float64_restatement_matches_the_wide_reference_goldens(case):
    z = np.load(os.path.join(G, f"restormer_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    assert cfg == gw.CASES[case]["cfg"] and int(z["seed"]) == gw.CASES[case]["seed"] and z["x"].shape == gw.CASES[case]["shape"]
    sd = {k: torch.from_numpy(v).double() for k, v in gw.make_state(cfg, int(z["seed"])).items()}
    x = gw.make_input(z["x"].shape, int(z["seed"]) + 1000)
    assert np.array_equal(x, z["x"])
    y = rt.restormer_forward(sd, torch.from_numpy(x).double(), **gw.full_cfg(**cfg)).numpy()
    assert np.abs(y - z["y64"]).max() < 1e-12
    # the reference's fp32 output is a few ulps from it: the bar the engine is held to on the GPU
    assert np.abs(z["y32"] - z["y64"]).max() < 1e-5


def test_model_cfg_dim_override_reaches_the_factory():
    from xmm_superres_denoise.config.config import MODELS_TOML, model_cfg
    from xmm_superres_denoise.models import Model
    assert MODELS_TOML["restormer"]["dim"] == 24           # the shipped entry is untouched
    m = Model(model_cfg("restormer", dim=48), (64, 64), (64, 64))
    m.configure_model()
    assert m.model.dim == 48 and m.model.decoder_level1[0].attn.qkv.in_channels == 96


def test_dim_with_another_model_is_refused_by_name_before_anything_is_read(tmp_path, monkeypatch, capsys):
    from xmm_superres_denoise import train
    from xmm_superres_denoise.infer import load_model
    missing = os.path.join(tmp_path, "no_such.ckpt")       # never opened: the refusal comes first
    for name in ("hat", "rrdb_denoise", "swinfir"):
        with pytest.raises(ValueError, match=f"{name}: dim=48 is not supported: dim is the width of 'restormer' only"):
            load_model(missing, name, dim=48)
    with pytest.raises(ValueError, match="hat: dim=48 is not supported"):
        train.test(missing, os.path.join(tmp_path, "no_such_dir"), name="hat", dim=48)
    monkeypatch.setattr(sys, "argv", ["train", "test", "--model", "hat", "--dim", "48", "--checkpoint", missing, "--dataset-dir", str(tmp_path)])
    with pytest.raises(SystemExit) as e:
        train.main()
    assert e.value.code == 2 and "hat: --dim 48 is not supported: dim is the width of `test --model restormer` only" in capsys.readouterr().err
    monkeypatch.setattr(sys, "argv", ["train", "fit", "--model", "restormer", "--dim", "48"])
    with pytest.raises(SystemExit):
        train.main()
    assert "--dim 48 is not supported" in capsys.readouterr().err


def test_speed_tool_prices_the_wide_kernels():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import restormer_speed as rs
    narrow, wide = rs.counts(1, 416, 416), rs.counts(1, 416, 416, rs.cfg_of(48))
    assert narrow["rst_wgram_kernel"][0] == 0 and narrow["rst_gram_kernel"][0] == narrow["rst_attn_kernel"][0] == 44
    # dim 48: the 4 + 4 blocks of decoder level 1 and the refinement are wide, the other 36 narrow
    assert [wide[k][0] for k in ("rst_wgram_kernel", "rst_wsoftmax_kernel", "rst_wfold_kernel", "rst_gram_kernel", "rst_attn_kernel")] == [8, 8, 8, 36, 36]
    # a wide Gram of 96 channels on one head at 416 x 416: q and k read twice (2 x 2 tiles), 169 double partials of 96^2 + 192 entries written
    HW, E = 416 * 416, 96 * 96 + 192
    assert wide["rst_wgram_kernel"][1] == 8 * 4.0 * (2 * 2 * 96 * HW + 2 * 169 * E)
    assert wide["rst_wgram_kernel"][2] == 8 * 2.0 * (96 * 96 + 2 * 96) * HW
