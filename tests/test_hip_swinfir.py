"""SwinFIR forward on the MI355X engine (csrc/swinfir.hip) through the drop-in module, against the reference's goldens and the float64
restatement (tests/golden/swinfir_torch.py): parity, the FourierUnit's FFT pair against torch.fft, batch isolation and determinism, the
Model / checkpoint / infer.py path, parameter re-packing, and the refusals (backward, H or W off the window grid, FFT sizes, fit)."""
import copy
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

import gen_swinfir as gs
import swinfir_torch as st

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _module(cfg, state, device="cuda"):
    from xmm_superres_denoise.models import SwinFIR
    m = SwinFIR(**gs.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return m.to(device)


def _sd(state, device, dtype):
    return {k: torch.from_numpy(v).to(device, dtype if v.dtype == np.float32 else None) for k, v in state.items()}


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


@pytest.mark.parametrize("case", list(gs.CASES))
def test_parity_with_reference_goldens(case):
    z = np.load(os.path.join(G, f"swinfir_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gs.make_state(cfg, int(z["seed"])))
    with torch.no_grad():
        y = m(torch.from_numpy(z["x"]).cuda()).cpu().numpy()
    assert y.shape == z["y64"].shape
    _assert_within_2x_of_fp32(y, z["y32"], z["y64"], case)


def test_full_size_xmm_configuration_416():
    """models.toml [swinfir] (19.0 M parameters, 13 x 13 windows, embed 180), one 416 x 416 tile -> 832 x 832, against the float64
    restatement run on the GPU; the fp32 yardstick is the same restatement in fp32 (torch eager) on the same device."""
    state = gs.make_state(gs.XMM, 2024)
    x = gs.make_input((1, 1, 416, 416), 2025)
    m = _module(gs.XMM, state)
    with torch.no_grad():
        y = m(torch.from_numpy(x).cuda()).cpu().numpy()
        y64 = st.swinfir_forward(_sd(state, "cuda", torch.float64), torch.from_numpy(x).cuda().double(), **gs.XMM).cpu().numpy()
        y32 = st.swinfir_forward(_sd(state, "cuda", torch.float32), torch.from_numpy(x).cuda(), **gs.XMM).cpu().numpy()
    assert y.shape == (1, 1, 832, 832)
    _assert_within_2x_of_fp32(y, y32, y64, "XMM configuration, 416 x 416")


@pytest.mark.parametrize("B,H,W,C2", [(1, 416, 416, 90), (2, 26, 39, 12), (1, 10, 15, 8), (2, 8, 8, 6), (1, 12, 18, 5)])
def test_fft_pair_against_torch_fft(B, H, W, C2):
    """the FourierUnit's transforms on their own: rfftn(ortho) and x + irfftn(s=(H, W), ortho) of a spectrum that is NOT Hermitian
    along H (as after the LeakyReLU) and has non-zero imaginary parts at the DC and Nyquist bins, against torch.fft in float64"""
    from xmm_superres_denoise.engine import SwinFIREngine
    eng = SwinFIREngine((16, 16), (1, 1), 1, 16, [1], [2], 4, 4.0, True, None, False, True, 2, 1.0, "pixelshuffle", "SFB")
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(B, H, W, C2, generator=g)
    spec = eng.fourier_pair(x.cuda()).cpu().double()
    ref = torch.fft.rfftn(x.double(), dim=(1, 2), norm="ortho")
    ref = torch.stack((ref.real, ref.imag), dim=-1)
    err = (spec - ref).abs().max().item() / ref.abs().max().item()
    s = torch.randn(B, H, W // 2 + 1, C2, 2, generator=g)
    back = eng.fourier_pair(x.cuda(), s.cuda()).cpu().double()
    sd = s.double()
    ref2 = x.double() + torch.fft.irfftn(torch.complex(sd[..., 0], sd[..., 1]), s=(H, W), dim=(1, 2), norm="ortho")
    err2 = (back - ref2).abs().max().item() / ref2.abs().max().item()
    print(f"{H} x {W}: rfftn max-rel {err:.2e}, x + irfftn max-rel {err2:.2e}")
    assert err < 2e-6 and err2 < 2e-6


def test_batch_isolation_determinism_and_nan_containment():
    z = np.load(os.path.join(G, "swinfir_b_shifted_odd_w.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gs.make_state(cfg, int(z["seed"])))
    x = torch.from_numpy(gs.make_input((4, 1, 10, 15), 77)).cuda()
    with torch.no_grad():
        y = m(x)
        y2 = m(x)
        singles = [m(x[i:i + 1].contiguous()) for i in range(4)]
        xn = x.clone()
        xn[2, 0, 7, 3] = float("nan")
        yn = m(xn)
    assert torch.equal(y, y2)                                      # two runs: bit for bit
    for i in range(4):
        assert torch.equal(y[i:i + 1], singles[i]), i              # each image = its own B = 1 run
    assert not torch.isfinite(yn[2]).all()
    for i in (0, 1, 3):
        assert torch.equal(yn[i], y[i]), i                         # the others do not see the NaN


def test_workspace_growth_and_replan_are_bitwise_neutral():
    """a larger shape after a smaller one (a larger workspace, new twiddles for H and a new plan), then the smaller one again (a re-plan inside the
    workspace held): neither leaves a trace in the outputs"""
    z = np.load(os.path.join(G, "swinfir_b_shifted_odd_w.npz"))
    cfg = json.loads(str(z["cfg"]))
    state = gs.make_state(cfg, int(z["seed"]))
    m, fresh = _module(cfg, state), _module(cfg, state)
    x1 = torch.from_numpy(gs.make_input((1, 1, 10, 15), 78)).cuda()
    x2 = torch.from_numpy(gs.make_input((2, 1, 20, 15), 79)).cuda()
    with torch.no_grad():
        y1, y2, y3 = m(x1), m(x2), m(x1)
        only2 = fresh(x2)                                          # a module that has only ever seen x2
    assert torch.equal(y1, y3)
    assert torch.equal(y2, only2)


def test_model_clamps_and_lightning_checkpoint_and_infer_file(tmp_path):
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.infer import infer_file, load_model, read_fits, write_fits
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.train import load_checkpoint
    cfg = model_cfg("swinfir")
    state = gs.make_state(gs.XMM, 31)
    ck = os.path.join(tmp_path, "swinfir.ckpt")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in state.items()}}, ck)
    model = Model(cfg, (416, 416), (832, 832))
    load_checkpoint(ck, model)
    model = model.cuda()
    x = torch.from_numpy(gs.make_input((1, 1, 416, 416), 32)).cuda()
    with torch.no_grad():
        raw = model.model(x)
        y = model(x)
    assert raw.shape == (1, 1, 832, 832)
    assert raw.min() < 0 or raw.max() > 1          # the module itself does not clamp (swinfir.py:441) ...
    assert torch.equal(y, raw.clamp(0, 1))         # ... Model.forward does (model.py:48-49)
    bare = os.path.join(tmp_path, "bare.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, bare)
    m2 = load_model(bare, "swinfir")
    with torch.no_grad():
        assert torch.equal(m2(x), y)
    counts = np.random.default_rng(5).poisson(0.3, size=(403, 411)).astype(np.float32)
    src = os.path.join(tmp_path, "P0001_detxy.fits")
    write_fits(src, counts, OrderedDict(CRPIX1=200.5, CRPIX2=204.5, CDELT1=-0.001, CDELT2=0.001, PA_PNT=12.5,
                                        EXPOSURE=10000.0))
    pred, out_path = infer_file(src, m2, None, os.path.join(tmp_path, "out"))
    back, h = read_fits(out_path)
    assert pred.shape == (832, 832) and np.isfinite(pred).all() and out_path.endswith("_sr_predict.fits.gz")
    assert np.array_equal(back.astype(np.float32), pred.astype(np.float32)) and h["CRPIX1"] == 2 * (200.5 + 6) + 0.5


def test_refusals_empty_batch_and_inference_mode():
    from xmm_superres_denoise.train import fit
    cfg = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=4, upsampler="pixelshuffle")
    m = _module(cfg, gs.make_state(cfg, 9))
    x = torch.from_numpy(gs.make_input((1, 1, 12, 16), 10)).cuda()
    y = m(x)                                       # grad mode on, parameters require grad: a graph node that refuses backward
    assert y.requires_grad and y.shape == (1, 1, 24, 32)
    with pytest.raises(RuntimeError, match="SwinFIR training is not on the MI355X engine"):
        y.sum().backward()
    with pytest.raises(RuntimeError, match="multiples of the window size 4"):
        m(torch.zeros(1, 1, 12, 18, device="cuda"))
    with pytest.raises(RuntimeError, match="FFT size 68 is not supported"):
        m(torch.zeros(1, 1, 68, 16, device="cuda"))             # 68 = 4 x 17: on the window grid, but 17 > 13
    with pytest.raises(NotImplementedError, match="swinfir"):
        fit("swinfir", steps=1)
    e = m(torch.zeros(0, 1, 12, 16, device="cuda"))
    assert e.shape == (0, 1, 24, 32)
    with torch.inference_mode():
        yi = m(x)
    with torch.no_grad():
        yn = m(x)
    assert torch.equal(yi, yn) and torch.equal(yn, y.detach())


def test_parameter_updates_repack_and_copies_are_independent():
    cfg = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=4, upsampler="pixelshuffle")
    state = gs.make_state(cfg, 11)
    m = _module(cfg, state)
    x = torch.from_numpy(gs.make_input((1, 1, 16, 16), 12)).cuda()

    def oracle(sd):
        return st.swinfir_forward({k: v.detach().cuda().double() if v.is_floating_point() else v.cuda() for k, v in sd.items()},
                                  x.double(), **cfg).float()

    with torch.no_grad():
        y0 = m(x)
        twin = copy.deepcopy(m)                     # a used module: the copy builds its own engine and flat buffer
        clone = pickle.loads(pickle.dumps(m))
        m.layers[0].residual_group.blocks[1].attn.qkv.weight.mul_(0.5)     # in-place updates (what an optimizer step does): re-packed
        m.layers[0].conv.F.fu.conv_layer.bias.add_(0.1)
        m.layers[0].residual_group.blocks[0].attn.relative_position_bias_table.add_(0.3)
        y1 = m(x)
        assert not torch.equal(y1, y0)
        assert (y1 - oracle(m.state_dict())).abs().max() < 1e-5
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
        assert torch.equal(m(x), y0)
        assert torch.equal(twin(x), y0) and torch.equal(clone.cuda()(x), y0)
