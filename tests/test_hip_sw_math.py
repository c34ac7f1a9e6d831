"""The opt-in bf16x6 math mode of the SwinFIR and HAT engines (csrc/sw_gemm_s3x.h): the GEMM / implicit-im2col 3x3 conv on its own in
both modes against float64, every golden of both networks under set_math("bf16x6"), switching between the modes, determinism, batch
isolation and NaN containment in bf16x6, and the plumbing of the mode through the modules, infer.load_model and train.test.

The bar throughout is the project's: rms and max-relative error against float64 at most 2x those of the fp32 yardstick (the golden's
y32, or the fp32 torch restatement on the same device).  A dropped mid or lo term of the split leaves errors near 2^-17, three orders
of magnitude outside it."""
import copy
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dataset_tree as dt
import gen_hat as gh
import gen_swinfir as gs

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -12345.0


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


def _act(y, act):
    return F.gelu(y) if act == "gelu" else F.leaky_relu(y, 0.01) if act == "lrelu" else y


def _check_gemm_modes(run, ref32, ref64, M, N, K, what):
    """both modes into a sentinel-filled [M + 3, N + 5] buffer: the bar, and nothing written past M rows or N columns"""
    outs = {}
    for math in ("fp32", "bf16x6"):
        buf = torch.full((M + 3, N + 5), SENTINEL, device="cuda")
        run(math, buf)
        assert torch.all(buf[M:] == SENTINEL) and torch.all(buf[:, N:] == SENTINEL), (what, math)
        outs[math] = buf[:M, :N].clone()
        _assert_within_2x_of_fp32(outs[math].cpu().numpy(), ref32, ref64, f"{what} {math}")
    if K >= 180:
        assert not torch.equal(outs["fp32"], outs["bf16x6"]), what      # the mode is really on
    return outs


@pytest.mark.parametrize("M,K,N,act", [(130, 20, 70, None), (257, 180, 540, None), (300, 720, 180, None), (64, 16, 1, None),
                                       (5, 7, 33, "gelu")])
def test_gemm_token_mode_against_float64(M, K, N, act):
    from xmm_superres_denoise.engine import sw_gemm
    g = torch.Generator().manual_seed(1000 * M + K)
    a = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    ref64 = _act(a.double() @ w.double().T + b.double(), act).cpu().numpy()
    ref32 = _act(a @ w.T + b, act).cpu().numpy()
    outs = _check_gemm_modes(lambda math, buf: sw_gemm(a, w, b, act=act, math=math, out=buf), ref32, ref64, M, N, K,
                             f"GEMM {M} x {K} x {N}")
    # without `out` and without a bias: a fresh [M, N] result, the same values minus the bias path
    y = sw_gemm(a, w, math="bf16x6")
    assert y.shape == (M, N)
    if act is None:
        _assert_within_2x_of_fp32(y.cpu().numpy(), (a @ w.T).cpu().numpy(), (a.double() @ w.double().T).cpu().numpy(), "no bias")
    assert torch.equal(sw_gemm(a, w, b, act=act, math="bf16x6"), outs["bf16x6"])        # two runs: bit for bit


@pytest.mark.parametrize("B,H,W,cin,N,act", [(2, 5, 7, 12, 33, None), (1, 9, 11, 180, 60, None), (3, 6, 6, 1, 16, None),
                                             (1, 16, 8, 60, 180, "lrelu")])
def test_conv3x3_mode_against_float64(B, H, W, cin, N, act):
    from xmm_superres_denoise.engine import sw_conv3x3
    g = torch.Generator().manual_seed(1000 * H + cin)
    x = torch.randn(B, H, W, cin, generator=g).cuda()
    w = (torch.randn(N, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    xn = x.permute(0, 3, 1, 2)

    def tok(y):
        return y.permute(0, 2, 3, 1).reshape(B * H * W, N).cpu().numpy()

    ref64 = tok(_act(F.conv2d(xn.double(), w.double(), b.double(), padding=1), act))
    ref32 = tok(_act(F.conv2d(xn.contiguous(), w, b, padding=1), act))
    _check_gemm_modes(lambda math, buf: sw_conv3x3(x, w, b, math=math, act=act, out=buf), ref32, ref64, B * H * W, N, 9 * cin,
                      f"conv3x3 {B} x {H} x {W}, {cin} -> {N}")
    y = sw_conv3x3(x, w, b, math="bf16x6", act=act)
    assert y.shape == (B, H, W, N)
    # each image of the batch equals its own B = 1 run: a 128-row tile that straddles two images mixes nothing
    for i in range(B):
        assert torch.equal(sw_conv3x3(x[i:i + 1].contiguous(), w, b, math="bf16x6", act=act)[0], y[i]), i


NETS = {"hat": (gh, "HAT"), "swinfir": (gs, "SwinFIR")}


def _module(net, cfg, state, device="cuda"):
    import xmm_superres_denoise.models as models
    gen, cls = NETS[net]
    m = getattr(models, cls)(**gen.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return m.to(device) if device else m


def _golden(net, case):
    z = np.load(os.path.join(G, f"{net}_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    return z, cfg, NETS[net][0].make_state(cfg, int(z["seed"]))


@pytest.mark.parametrize("net,case", [("hat", c) for c in gh.CASES] + [("swinfir", c) for c in gs.CASES])
def test_goldens_in_bf16x6_and_switching_modes(net, case):
    z, cfg, state = _golden(net, case)
    m, fresh = _module(net, cfg, state), _module(net, cfg, state)
    x = torch.from_numpy(z["x"]).cuda()
    with torch.no_grad():
        want32 = fresh(x)                               # a module that never left fp32
        a32 = m(x)
        b6 = m.set_math("bf16x6")(x)
        assert m._engine.get_math() == "bf16x6"
        c32 = m.set_math("fp32")(x)
        d6 = m.set_math("bf16x6")(x)
    _assert_within_2x_of_fp32(b6.cpu().numpy(), z["y32"], z["y64"], f"{net} {case} bf16x6")
    assert torch.equal(a32, want32) and torch.equal(c32, want32)
    assert torch.equal(d6, b6)
    assert fresh._engine.get_math() == "fp32"


@pytest.mark.parametrize("net,case,shape", [("hat", "a_shifted_ocab", (4, 1, 16, 24)), ("swinfir", "b_shifted_odd_w", (4, 1, 10, 15))])
def test_bf16x6_determinism_batch_isolation_nan_and_repack(net, case, shape):
    z, cfg, state = _golden(net, case)
    m = _module(net, cfg, state).set_math("bf16x6")
    x = torch.from_numpy(NETS[net][0].make_input(shape, 77)).cuda()
    with torch.no_grad():
        y = m(x)
        y2 = m(x)
        singles = [m(x[i:i + 1].contiguous()) for i in range(4)]
        xn = x.clone()
        xn[2, 0, 7, 3] = float("nan")
        yn = m(xn)
        assert m._engine.get_math() == "bf16x6"
        assert torch.equal(y, y2)                                      # two runs: bit for bit
        for i in range(4):
            assert torch.equal(y[i:i + 1], singles[i]), i              # each image = its own B = 1 run
        assert not torch.isfinite(yn[2]).all()
        for i in (0, 1, 3):
            assert torch.equal(yn[i], y[i]), i                         # the others do not see the NaN
        # a parameter edit is picked up: the bf16 planes follow the repack, and the result is what a fresh module of the edited
        # parameters computes
        m.conv_after_body.weight.mul_(0.5)
        m.layers[0].residual_group.blocks[0].mlp.fc1.weight.add_(0.01)
        y3 = m(x)
        assert not torch.equal(y3, y)
        twin = _module(net, cfg, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}).set_math("bf16x6")
        assert torch.equal(twin(x), y3)


def test_mode_plumbing_through_the_modules(monkeypatch):
    from xmm_superres_denoise.engine import HATEngine, RestormerEngine, XsdError
    z, cfg, state = _golden("hat", "a_shifted_ocab")
    x = torch.from_numpy(z["x"]).cuda()
    m = _module("hat", cfg, state, device=None)
    assert m.get_math() == "fp32"
    m.set_math("bf16x6")                                # before .cuda(): remembered, applied when the engine is made
    assert m._engine is None and m.get_math() == "bf16x6"
    m = m.cuda()
    with torch.no_grad():
        y = m(x)
        assert m._engine.get_math() == "bf16x6"
        for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)).cuda()):
            assert other._engine is None and other.get_math() == "bf16x6"
            assert torch.equal(other(x), y) and other._engine.get_math() == "bf16x6"
    # the environment variable of the RRDB engine is not read here
    monkeypatch.setenv("XSD_MATH", "bf16x6")
    eng = HATEngine((16, 16), (1, 1), 1, 16, [2], [2], 4, 3, 4, 0.5, 0.5, 2.0, True, None, False, True, 2, 1.0, "pixelshuffle", "1conv")
    assert eng.get_math() == "fp32"
    with pytest.raises(XsdError, match="per-tensor scale"):
        eng.set_math("f16x3")
    with pytest.raises(XsdError, match=r"unknown math mode 'tf32'.*bf16x6.*fp32"):
        eng.set_math("tf32")
    # the C side says the same to a caller that bypasses the wrapper
    assert eng.L.xsd_hat_set_math(eng.h, 4) != 0 and b"per-tensor scale" in eng.L.xsd_last_error()
    assert eng.L.xsd_hat_set_math(eng.h, 7) != 0 and b"fp32 (0) and bf16x6 (3)" in eng.L.xsd_last_error()
    assert eng.get_math() == "fp32"
    eng.set_math("bf16x6")
    assert eng.get_math() == "bf16x6"
    r = RestormerEngine(1, 1, 8, [1, 1, 1, 1], 1, [1, 2, 4, 8], 2.66, False, False)
    with pytest.raises(XsdError, match="Restormer: math mode 'bf16x6' is not supported"):
        r.set_math("bf16x6")
    r.set_math("fp32")
    assert r.get_math() == "fp32"


def test_load_model_infer_file_and_train_test_take_the_mode(tmp_path):
    """infer.load_model(math=) + infer_file and train.test(math=) on a tiny synthetic FITS tree: the full XMM HAT configuration on small
    tiles (lr_res 64 -> 128), the same keys with and without the flag"""
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.data.datamodule import XmmDataModule
    from xmm_superres_denoise.infer import infer_file, load_model, write_fits
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.train import dataset_cfg, test
    root = dt.make_sim_tree(str(tmp_path / "tree"), n_base=10, n_agn=2, n_bkg=2, lr_exps=(20,), hr_exp=50, hr_mult=2, shape=(60, 52), seed=3)
    run = tmp_path / "run"
    os.makedirs(run)
    ck = str(run / "hat.ckpt")
    torch.manual_seed(4)
    model = Model(model_cfg("hat"), (192, 192), (384, 384))
    model.configure_model(forward_only_hat=True)
    torch.save({"state_dict": {"model." + k: v for k, v in model.model.state_dict().items()}}, ck)
    m6 = load_model(ck, "hat", lr_res=192, math="bf16x6")
    assert m6.model.get_math() == "bf16x6"
    counts = np.random.default_rng(5).poisson(0.3, size=(180, 170)).astype(np.float32)
    src = os.path.join(tmp_path, "P0001_detxy.fits")
    write_fits(src, counts, OrderedDict(CRPIX1=90.5, CRPIX2=85.5, CDELT1=-0.001, CDELT2=0.001, PA_PNT=12.5, EXPOSURE=10000.0))
    pred, out_path = infer_file(src, m6, None, os.path.join(tmp_path, "out"), lr_res=192)
    assert pred.shape == (384, 384) and np.isfinite(pred).all() and m6.model._engine.get_math() == "bf16x6"
    pred32, _ = infer_file(src, load_model(ck, "hat", lr_res=192), None, os.path.join(tmp_path, "out32"), lr_res=192)
    assert pred32.shape == pred.shape and not np.array_equal(pred, pred32)        # the mode reached the engine
    dcfg = dataset_cfg(root, name="hat", lr_res=192, hr_exp=50, batch_size=2)
    splits = str(run / f"{dcfg.name}_{dcfg.type}_{dcfg.mode}_splits.json")
    XmmDataModule(dcfg, splits, seed=2).prepare_data()
    plain = test(ck, root, name="hat", lr_res=192, hr_exp=50, batch_size=2, log=False)
    got = test(ck, root, name="hat", lr_res=192, hr_exp=50, batch_size=2, log=False, math="bf16x6")
    assert set(got) == set(plain) and all(np.isfinite(v) for v in got.values()), got
    with pytest.raises(ValueError, match="restormer: math mode 'bf16x6' is not supported"):
        load_model(ck, "restormer", lr_res=192, math="bf16x6")
