"""Restormer forward on the MI355X engine (csrc/restormer.hip) through the drop-in module, against the reference's goldens and the
float64 restatement (tests/golden/restormer_torch.py): parity, batch isolation and determinism, the Model / checkpoint / infer.py
path, parameter re-packing, and the refusals (backward, H or W not divisible by 8, dual_pixel_task)."""
import copy
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

import gen_restormer as gr
import restormer_torch as rt

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _module(cfg, state, device="cuda"):
    from xmm_superres_denoise.models import Restormer
    m = Restormer(**gr.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return m.to(device)


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


@pytest.mark.parametrize("case", list(gr.CASES))
def test_parity_with_reference_goldens(case):
    z = np.load(os.path.join(G, f"restormer_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gr.make_state(cfg, int(z["seed"])))
    with torch.no_grad():
        y = m(torch.from_numpy(z["x"]).cuda()).cpu().numpy()
    assert y.shape == z["y64"].shape
    _assert_within_2x_of_fp32(y, z["y32"], z["y64"], case)


def test_full_size_xmm_configuration_416():
    """dim = 24 with the reference's default depths and heads (models.toml:58-64), one 416 x 416 tile, against the float64
    restatement run on the GPU; the fp32 yardstick is the same restatement in fp32 (torch eager) on the same device."""
    cfg = dict(inp_channels=1, out_channels=1, dim=24)
    state = gr.make_state(cfg, 2024)
    x = gr.make_input((1, 1, 416, 416), 2025)
    m = _module(cfg, state)
    with torch.no_grad():
        y = m(torch.from_numpy(x).cuda()).cpu().numpy()
        full = gr.full_cfg(**cfg)
        sd64 = {k: torch.from_numpy(v).cuda().double() for k, v in state.items()}
        y64 = rt.restormer_forward(sd64, torch.from_numpy(x).cuda().double(), **full).cpu().numpy()
        sd32 = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
        y32 = rt.restormer_forward(sd32, torch.from_numpy(x).cuda(), **full).cpu().numpy()
    _assert_within_2x_of_fp32(y, y32, y64, "dim 24, 416 x 416")


def test_batch_isolation_determinism_and_nan_containment():
    z = np.load(os.path.join(G, "restormer_a_dim8_default.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gr.make_state(cfg, int(z["seed"])))
    x = torch.from_numpy(gr.make_input((4, 3, 32, 40), 77)).cuda()
    with torch.no_grad():
        y = m(x)
        y2 = m(x)
        singles = [m(x[i:i + 1].contiguous()) for i in range(4)]
        xn = x.clone()
        xn[2, 1, 17, 5] = float("nan")
        yn = m(xn)
    assert torch.equal(y, y2)                                      # two runs: bit for bit
    for i in range(4):
        assert torch.equal(y[i:i + 1], singles[i]), i              # each image = its own B = 1 run
    assert not torch.isfinite(yn[2]).all()
    for i in (0, 1, 3):
        assert torch.equal(yn[i], y[i]), i                         # the others do not see the NaN


def test_model_clamps_and_lightning_checkpoint_and_infer_file(tmp_path):
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.infer import infer_file, load_model, read_fits, write_fits
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.train import load_checkpoint
    cfg = model_cfg("restormer")
    state = gr.make_state(dict(inp_channels=1, out_channels=1, dim=24), 31)
    # a Lightning-layout checkpoint ("model." + the reference's key names), as the reference's trainer writes it
    ck = os.path.join(tmp_path, "restormer.ckpt")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in state.items()}}, ck)
    model = Model(cfg, (416, 416), (416, 416))
    load_checkpoint(ck, model)
    model = model.cuda()
    x = torch.from_numpy(gr.make_input((1, 1, 416, 416), 32)).cuda()
    with torch.no_grad():
        raw = model.model(x)
        y = model(x)
    assert raw.min() < 0 or raw.max() > 1          # the module itself does not clamp (restormer.py:404) ...
    assert torch.equal(y, raw.clamp(0, 1))         # ... Model.forward does (model.py:48-49)
    # infer.py: FITS in -> Restormer checkpoint -> FITS out (the rrdb_denoise path); a bare state_dict loads too
    bare = os.path.join(tmp_path, "bare.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, bare)
    m2 = load_model(bare, "restormer")
    counts = np.random.default_rng(5).poisson(0.3, size=(403, 411)).astype(np.float32)
    src = os.path.join(tmp_path, "P0001_detxy.fits")
    write_fits(src, counts, OrderedDict(CRPIX1=200.5, CRPIX2=204.5, EXPOSURE=10000.0))
    pred, out_path = infer_file(src, m2, None, os.path.join(tmp_path, "out"))
    back, h = read_fits(out_path)
    assert pred.shape == (416, 416) and np.isfinite(pred).all() and out_path.endswith("_dn_predict.fits.gz")
    assert np.array_equal(back.astype(np.float32), pred.astype(np.float32)) and h["CRPIX1"] == 206.5


def test_refusals_empty_batch_and_inference_mode():
    from xmm_superres_denoise.models import Restormer
    cfg = dict(inp_channels=1, out_channels=1, dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1)
    m = _module(cfg, gr.make_state(cfg, 9))
    x = torch.from_numpy(gr.make_input((1, 1, 16, 24), 10)).cuda()
    y = m(x)                                       # grad mode on, parameters require grad: a graph node that refuses backward
    assert y.requires_grad
    with pytest.raises(RuntimeError, match="Restormer training is not on the MI355X engine"):
        y.sum().backward()
    with pytest.raises(RuntimeError, match="divisible by 8"):
        m(torch.zeros(1, 1, 20, 24, device="cuda"))
    with pytest.raises(ValueError, match="dual_pixel_task"):
        Restormer(6, 3, 8, dual_pixel_task=True)
    e = m(torch.zeros(0, 1, 16, 24, device="cuda"))
    assert e.shape == (0, 1, 16, 24)
    with torch.inference_mode():
        yi = m(x)
    with torch.no_grad():
        yn = m(x)
    assert torch.equal(yi, yn) and torch.equal(yn, y.detach())


def test_parameter_updates_repack_and_copies_are_independent():
    cfg = dict(inp_channels=1, out_channels=1, dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, bias=True)
    state = gr.make_state(cfg, 11)
    m = _module(cfg, state)
    x = torch.from_numpy(gr.make_input((1, 1, 16, 16), 12)).cuda()
    full = gr.full_cfg(**cfg)

    def oracle(sd):
        return rt.restormer_forward({k: v.detach().cuda().double() for k, v in sd.items()}, x.double(), **full).float()

    with torch.no_grad():
        y0 = m(x)
        twin = copy.deepcopy(m)                     # a used module: the copy builds its own engine and flat buffer
        clone = pickle.loads(pickle.dumps(m))
        m.encoder_level1[0].attn.qkv.weight.mul_(0.5)        # an in-place update (what an optimizer step does): re-packed
        m.latent[0].ffn.project_in.bias.add_(0.1)
        y1 = m(x)
        assert (y1 - oracle(m.state_dict())).abs().max() < 1e-4
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
        assert torch.equal(m(x), y0)
        assert torch.equal(twin(x), y0) and torch.equal(clone.cuda()(x), y0)
