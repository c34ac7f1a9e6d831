"""HAT forward on the MI355X engine (csrc/hat.hip) through the drop-in module, against the reference's goldens and the float64
restatement (tests/golden/hat_torch.py): parity, the overlapping cross-attention and the channel attention's pool on their own, batch
isolation and determinism, the Model / checkpoint / infer.py / train.test path, parameter re-packing, and the refusals (backward, H or W
off the window grid, fit)."""
import copy
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dataset_tree as dt
import gen_hat as gh
import hat_torch as ht

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

SMALL = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=4, squeeze_factor=4,
             conv_scale=0.5, upsampler="pixelshuffle")


def _module(cfg, state, device="cuda"):
    from xmm_superres_denoise.models import HAT
    m = HAT(**gh.full_cfg(**cfg))
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


@pytest.mark.parametrize("case", list(gh.CASES))
def test_parity_with_reference_goldens(case):
    z = np.load(os.path.join(G, f"hat_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gh.make_state(cfg, int(z["seed"])))
    with torch.no_grad():
        y = m(torch.from_numpy(z["x"]).cuda()).cpu().numpy()
    assert y.shape == z["y64"].shape
    _assert_within_2x_of_fp32(y, z["y32"], z["y64"], case)


def test_full_size_xmm_configuration_416():
    """models.toml [hat] at full depth (26.1 M parameters, 6 x (6 HABs + 1 OCAB), 16 x 16 windows against 24 x 24 keys, embed 180), one
    416 x 416 tile -> 832 x 832, against the float64 restatement run on the GPU; the fp32 yardstick is the same restatement in fp32
    (torch eager) on the same device."""
    state = gh.make_state(gh.XMM, 2024)
    x = gh.make_input((1, 1, 416, 416), 2025)
    m = _module(gh.XMM, state)
    with torch.no_grad():
        y = m(torch.from_numpy(x).cuda()).cpu().numpy()
        y64 = ht.hat_forward(_sd(state, "cuda", torch.float64), torch.from_numpy(x).cuda().double(), **gh.XMM).cpu().numpy()
        y32 = ht.hat_forward(_sd(state, "cuda", torch.float32), torch.from_numpy(x).cuda(), **gh.XMM).cpu().numpy()
    assert y.shape == (1, 1, 832, 832)
    _assert_within_2x_of_fp32(y, y32, y64, "XMM configuration, 416 x 416")


@pytest.mark.parametrize("B,H,W,C,heads,ws,ow", [(1, 48, 64, 180, 6, 16, 24), (2, 10, 15, 32, 2, 5, 7), (1, 8, 8, 24, 3, 8, 12),
                                                 (1, 12, 8, 16, 2, 4, 4)])
def test_overlapping_cross_attention_against_float64(B, H, W, C, heads, ws, ow):
    """the OCAB's attention on its own against hat_torch.ocab_attention in float64: the whole image (its border windows take the
    zero-padded keys, which enter the softmax with score = bias) and the interior windows alone; the yardstick is the same
    restatement in fp32 eager, the bar the project's 2x"""
    from xmm_superres_denoise.engine import hat_ocab_attention
    g = torch.Generator().manual_seed(1000 * H + W)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).cuda()
    table = (torch.rand((ws + ow - 1) ** 2, heads, generator=g) - 0.5).cuda()
    scale = (C // heads) ** -0.5
    o = hat_ocab_attention(qkv, table, H, W, heads, ws, ow, scale).cpu().numpy()
    o64 = ht.ocab_attention(qkv.double(), table.double(), H, W, heads, ws, ow, scale).cpu().numpy()
    o32 = ht.ocab_attention(qkv, table, H, W, heads, ws, ow, scale).cpu().numpy()
    _assert_within_2x_of_fp32(o, o32, o64, f"OCAB {H} x {W}, window {ws} / {ow}, whole image")
    if H >= 3 * ws and W >= 3 * ws:
        def inner(a):
            return a.reshape(B, H, W, C)[:, ws:H - ws, ws:W - ws]
        _assert_within_2x_of_fp32(inner(o), inner(o32), inner(o64), f"OCAB {H} x {W}, window {ws} / {ow}, interior windows")


@pytest.mark.parametrize("HW,C", [(416 * 416, 180), (150, 32), (1000, 7)])
def test_channel_attention_pool_is_exact_and_batch_independent(HW, C):
    """the pooled means equal x.double().mean over the pixels to fp32 rounding, and are bitwise equal between B = 1 and B = 4"""
    from xmm_superres_denoise.engine import hat_channel_mean
    g = torch.Generator().manual_seed(HW + C)
    x = (torch.randn(4, HW, C, generator=g) * 3 + 0.7).cuda()
    m4 = hat_channel_mean(x)
    want = x.double().mean(1)
    # rounding the double mean to fp32 costs at most 2^-24 |mean| <= 2^-24 mean|x|; the double sums differ from torch's by about
    # HW 2^-53 mean|x|, which can move a mean on a rounding boundary to the neighbouring float: 2^-23 mean|x| bounds both, also for a
    # channel whose mean is near zero
    rel = ((m4.double() - want).abs() / x.double().abs().mean(1)).max().item()
    print(f"pool {HW} x {C}: max err of the means relative to mean|x| {rel:.2e}")
    assert rel <= 2.0 ** -23
    for i in range(4):
        assert torch.equal(hat_channel_mean(x[i:i + 1].contiguous())[0], m4[i]), i


def test_batch_isolation_determinism_and_nan_containment():
    z = np.load(os.path.join(G, "hat_a_shifted_ocab.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gh.make_state(cfg, int(z["seed"])))
    x = torch.from_numpy(gh.make_input((4, 1, 16, 24), 77)).cuda()
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
    """a larger shape after a smaller one (a larger workspace and a new plan), then the smaller one again (a re-plan inside the
    workspace held): neither leaves a trace in the outputs"""
    z = np.load(os.path.join(G, "hat_a_shifted_ocab.npz"))
    cfg = json.loads(str(z["cfg"]))
    state = gh.make_state(cfg, int(z["seed"]))
    m, fresh = _module(cfg, state), _module(cfg, state)
    x1 = torch.from_numpy(gh.make_input((1, 1, 16, 24), 78)).cuda()
    x2 = torch.from_numpy(gh.make_input((2, 1, 32, 24), 79)).cuda()
    with torch.no_grad():
        y1, y2, y3 = m(x1), m(x2), m(x1)
        only2 = fresh(x2)                                          # a module that has only ever seen x2
    assert torch.equal(y1, y3)
    assert torch.equal(y2, only2)


def test_model_clamps_and_lightning_checkpoint_and_infer_file(tmp_path):
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.infer import infer_file, load_model, read_fits, write_fits
    from xmm_superres_denoise.models import HAT, Model
    from xmm_superres_denoise.train import load_checkpoint
    cfg = model_cfg("hat")
    state = gh.make_state(gh.XMM, 31)
    ck = os.path.join(tmp_path, "hat.ckpt")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in state.items()}}, ck)
    model = Model(cfg, (416, 416), (832, 832))
    model.configure_model(forward_only_hat=True)
    load_checkpoint(ck, model)
    model = model.cuda()
    x = torch.from_numpy(gh.make_input((1, 1, 416, 416), 32)).cuda()
    with torch.no_grad():
        raw = model.model(x)
        y = model(x)
    assert isinstance(model.model, HAT) and raw.shape == (1, 1, 832, 832)
    assert raw.min() < 0 or raw.max() > 1          # the module itself does not clamp (hat.py:911-913) ...
    assert torch.equal(y, raw.clamp(0, 1))         # ... Model.forward does (model.py:48-49)
    bare = os.path.join(tmp_path, "bare.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, bare)
    m2 = load_model(bare, "hat")
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


def test_train_test_routine_runs_hat(tmp_path, capsys):
    """`train test --model hat` on a tiny synthetic FITS tree, with and without the extended metrics.  The model is the FULL XMM
    configuration (models.toml [hat], 26.1 M parameters, default initialisation); only the tiles are small (lr_res 320 -> 640)."""
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.data.datamodule import XmmDataModule
    from xmm_superres_denoise.metrics.xmm_metric_collection import EXT_NAMES, NAMES
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.train import dataset_cfg, test
    root = dt.make_sim_tree(str(tmp_path / "tree"), n_base=10, n_agn=2, n_bkg=2, lr_exps=(20,), hr_exp=50, hr_mult=2, shape=(60, 52), seed=3)
    run = tmp_path / "run"
    os.makedirs(run)
    ck = str(run / "hat.ckpt")
    torch.manual_seed(4)
    model = Model(model_cfg("hat"), (320, 320), (640, 640))
    model.configure_model(forward_only_hat=True)
    torch.save({"state_dict": {"model." + k: v for k, v in model.model.state_dict().items()}}, ck)
    dcfg = dataset_cfg(root, name="hat", lr_res=320, hr_exp=50, batch_size=2)
    assert dcfg.hr.res == 640
    splits = str(run / f"{dcfg.name}_{dcfg.type}_{dcfg.mode}_splits.json")
    XmmDataModule(dcfg, splits, seed=2).prepare_data()             # fit would write it; fit refuses HAT
    old = {"test/loss"} | {f"test/linear/{n}" for n in NAMES} | {f"test/linear/in/{n}" for n in NAMES}
    ext = {f"test/linear/{n}" for n in EXT_NAMES} | {f"test/linear/in/{n}" for n in EXT_NAMES}
    plain = test(ck, root, name="hat", lr_res=320, hr_exp=50, batch_size=2)
    assert set(plain) == old and all(np.isfinite(v) for v in plain.values()), plain
    got = test(ck, root, name="hat", lr_res=320, hr_exp=50, batch_size=2, extended_metrics=True)
    out = capsys.readouterr().out
    assert set(got) == old | ext and all(np.isfinite(v) for v in got.values()), got
    assert "fsim is the only metric left out" in out
    for k in old:
        assert plain[k] == got[k], k


def test_refusals_empty_batch_and_inference_mode():
    from xmm_superres_denoise.train import fit
    m = _module(SMALL, gh.make_state(SMALL, 9))
    x = torch.from_numpy(gh.make_input((1, 1, 12, 16), 10)).cuda()
    y = m(x)                                       # grad mode on, parameters require grad: a graph node that refuses backward
    assert y.requires_grad and y.shape == (1, 1, 24, 32)
    with pytest.raises(RuntimeError, match="HAT training is not on the MI355X engine"):
        y.sum().backward()
    with pytest.raises(RuntimeError, match="multiples of the window size 4"):
        m(torch.zeros(1, 1, 12, 18, device="cuda"))
    with pytest.raises(RuntimeError, match="multiples of the window size 4"):
        m(torch.zeros(1, 1, 10, 16, device="cuda"))
    with pytest.raises(NotImplementedError, match="hat: training HAT is not on the MI355X engine"):
        fit("hat", steps=1)
    e = m(torch.zeros(0, 1, 12, 16, device="cuda"))
    assert e.shape == (0, 1, 24, 32)
    with torch.inference_mode():
        yi = m(x)
    with torch.no_grad():
        yn = m(x)
    assert torch.equal(yi, yn) and torch.equal(yn, y.detach())


def test_parameter_updates_repack_and_copies_are_independent():
    state = gh.make_state(SMALL, 11)
    m = _module(SMALL, state)
    x = torch.from_numpy(gh.make_input((1, 1, 16, 16), 12)).cuda()

    def oracle(sd):
        return ht.hat_forward({k: v.detach().cuda().double() if v.is_floating_point() else v.cuda() for k, v in sd.items()},
                              x.double(), **SMALL).float()

    with torch.no_grad():
        y0 = m(x)
        assert (y0 - oracle(m.state_dict())).abs().max() < 1e-5
        twin = copy.deepcopy(m)                     # a used module: the copy builds its own engine and flat buffer
        clone = pickle.loads(pickle.dumps(m))
        g = m.layers[0].residual_group
        for edit in (lambda: g.blocks[1].attn.qkv.weight.mul_(0.5),                    # in-place updates (what an optimizer step does)
                     lambda: g.blocks[0].conv_block.cab[3].attention[3].bias.add_(2.0),   # read as stored, never packed
                     lambda: g.overlap_attn.relative_position_bias_table.add_(torch.linspace(-1, 1, 81 * 2, device="cuda").view(81, 2))):
            before = m(x)
            edit()
            after = m(x)
            assert not torch.equal(after, before)
            assert (after - oracle(m.state_dict())).abs().max() < 1e-5
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
        assert torch.equal(m(x), y0)
        assert torch.equal(twin(x), y0) and torch.equal(clone.cuda()(x), y0)
