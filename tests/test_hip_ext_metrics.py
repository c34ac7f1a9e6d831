"""The extended test metrics on the MI355X (csrc/ext_metrics.hip, xsd_ext_metrics_eval): gmsd, ms_gmsd, haarpsi, msdi, vif_p.

The comparator is the plain-torch restatement tests/golden/ext_metrics_torch.py on the CPU -- this project's specification of the
metrics, restated from the published code of piq 0.7.x and torchmetrics 1.x.  PARITY WITH THE LIBRARIES THEMSELVES IS UNPINNED
(neither is available here), exactly as for psnr / ssim / ms_ssim.

Accuracy rule, per metric and image:  |engine - f64| <= max(2 * |f32 - f64|, 5e-6 * max(1, |f64|)),  f32 / f64 = the restatement
in the two dtypes on the same fp32-representable inputs: twice the reference arithmetic's own error (the rule of
test_hip_restormer.py), with test_hip_loss.py's 5e-6 bar as the floor for cases where fp32 happens to be exact."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_tree as dt
import ext_metrics_torch as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES = {"416x416": (416, 416), "832x832": (832, 832), "61x53": (61, 53), "417x403": (417, 403)}
_cache = {}


def _named(out):
    """engine result [B, 6] -> {name: [B]} (CPU doubles)"""
    out = out.cpu()
    return {"gmsd": out[:, 0], "ms_gmsd": out[:, 1], "haarpsi": out[:, 2], "msdi": out[:, 3], "vif_p": out[:, 4] / out[:, 5]}


def _case(size):
    """four seeded photon-like pairs of the size, rounded to fp32 (so the engine and both restatements see the same numbers), and
    the restatement's values in float64 and float32"""
    if size not in _cache:
        H, W = SIZES[size]
        p, t = E.photon_pair((4, H, W), torch.Generator().manual_seed(100 + H + W))
        p, t = p.float(), t.float()
        m64, m32 = E.all_metrics(p.double(), t.double()), E.all_metrics(p, t)
        # vif_p's numerator and denominator on their own too: an error common to both cancels in the ratio
        m64["vif_num"], m64["vif_den"] = E.vif_parts(p.double(), t.double())
        m32["vif_num"], m32["vif_den"] = E.vif_parts(p, t)
        _cache[size] = (p, t, m64, m32)
    return _cache[size]


def _bar(f32, f64):
    return max(2 * abs(f32 - f64), 5e-6 * max(1.0, abs(f64)))


@pytest.fixture(scope="module")
def engine():
    from xmm_superres_denoise.engine import ExtMetricsEngine
    with torch.cuda.device(DEV):
        return ExtMetricsEngine()


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("size", list(SIZES))
def test_accuracy_against_the_float64_restatement(engine, size, B):
    p, t, m64, m32 = _case(size)
    out = engine.eval(p[:B].to(DEV), t[:B].to(DEV))
    got = _named(out)
    got["vif_num"], got["vif_den"] = out[:, 4].cpu(), out[:, 5].cpu()
    misses = []
    for n in E.NAMES + ("vif_num", "vif_den"):
        for b in range(B):
            g, f64, f32 = got[n][b].item(), m64[n][b].item(), float(m32[n][b].item())
            bar = _bar(f32, f64)
            print(f"{size} B={B} image {b} {n:8s} f64 {f64:.10f} engine {g:.10f} |engine-f64| {abs(g - f64):.2e} |f32-f64| {abs(f32 - f64):.2e} bar {bar:.2e}")
            if not abs(g - f64) <= bar:
                misses.append((n, b, g, f64, f32))
    assert not misses, misses


def test_batch_independence_and_determinism_bitwise(engine):
    for size in ("416x416", "61x53"):
        p, t = (a.to(DEV) for a in _case(size)[:2])
        a = engine.eval(p, t)
        assert torch.equal(a, engine.eval(p, t))
        singles = torch.cat([engine.eval(p[i:i + 1].contiguous(), t[i:i + 1].contiguous()) for i in range(4)])
        assert torch.equal(a, singles)
        # a [B, 1, H, W] tensor is the same batch
        assert torch.equal(a, engine.eval(p[:, None], t[:, None]))
        # another engine object, other batch-mates, another order
        from xmm_superres_denoise.engine import ExtMetricsEngine
        b = ExtMetricsEngine().eval(p.flip(0).contiguous(), t.flip(0).contiguous())
        assert torch.equal(a, b.flip(0))


@pytest.mark.parametrize("where", ["preds", "target"])
def test_nan_pixel_stays_in_its_image(engine, where):
    p, t, _, _ = _case("61x53")
    clean = engine.eval(p.to(DEV), t.to(DEV))
    p, t = p.clone(), t.clone()
    (p if where == "preds" else t)[2, 30, 17] = float("nan")
    got = engine.eval(p.to(DEV), t.to(DEV))
    assert torch.equal(got[[0, 1, 3]], clean[[0, 1, 3]])
    want = E.all_metrics(p.double(), t.double())
    g = _named(got)
    for n in E.NAMES:
        assert bool(torch.isfinite(g[n][2])) == bool(torch.isfinite(want[n][2])), n
        assert not torch.isfinite(g[n][2]), n          # (every one of the five sees every pixel)


def test_constant_target_gives_nan_vif_as_written(engine):
    p, t, _, _ = _case("61x53")
    t = t.clone()
    t[1] = 0.25
    got = _named(engine.eval(p.to(DEV), t.to(DEV)))
    want = E.all_metrics(p.double(), t.double())
    assert torch.isnan(want["vif_p"][1]) and torch.isnan(got["vif_p"][1])        # 0 / 0, torchmetrics as written
    for n in ("gmsd", "ms_gmsd", "haarpsi", "msdi"):
        assert abs(got[n][1].item() - want[n][1].item()) <= 5e-6 * max(1.0, abs(want[n][1].item())), n
    for n in E.NAMES:
        assert torch.isfinite(got[n][[0, 2, 3]]).all()


def test_refusals(engine):
    from xmm_superres_denoise.engine import XsdError, _lib
    z = torch.zeros((1, 64, 64), device=DEV)
    for shape in ((1, 40, 64), (1, 64, 40), (2, 17, 17)):
        with pytest.raises(XsdError, match="41"):
            engine.eval(torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV))
    engine.eval(torch.zeros((1, 41, 41), device=DEV), torch.zeros((1, 41, 41), device=DEV))       # the smallest size is taken
    with pytest.raises(XsdError, match="shape mismatch"):
        engine.eval(z, torch.zeros((1, 64, 65), device=DEV))
    with pytest.raises(XsdError, match="no CPU fallback"):
        engine.eval(z.cpu(), z.cpu())
    with pytest.raises(XsdError, match="float32"):
        engine.eval(z.double(), z.double())
    with pytest.raises(XsdError, match=r"\[B,H,W\]"):
        engine.eval(torch.zeros((1, 2, 64, 64), device=DEV), torch.zeros((1, 2, 64, 64), device=DEV))
    L = _lib.load()
    out = torch.zeros((1, 6), dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert L.xsd_ext_metrics_eval(engine.h, z.data_ptr(), z.data_ptr(), out.data_ptr(), 0, 64, 64, stream) == -1
    assert b"B must be" in L.xsd_last_error()
    for args in ((None, z.data_ptr(), z.data_ptr(), out.data_ptr()), (engine.h, None, z.data_ptr(), out.data_ptr()),
                 (engine.h, z.data_ptr(), None, out.data_ptr()), (engine.h, z.data_ptr(), z.data_ptr(), None)):
        assert L.xsd_ext_metrics_eval(*args, 1, 64, 64, stream) == -1
        assert b"null pointer" in L.xsd_last_error()
    assert L.xsd_ext_metrics_create(None) == -1
    L.xsd_ext_metrics_destroy(None)
    torch.cuda.synchronize()


def _expected_epoch(batches, dataset_norm, scaling, names_prefix=""):
    """the collection's values from the restatement: per batch denorm -> renorm on the device (the engine's own stretch kernels,
    tested elsewhere), the restatement in float64 / float32 on the CPU, the reference's epoch reduction"""
    out64, out32 = {}, {}
    for n in scaling:
        per64, per32 = [], []
        for p, t in batches:
            pp, tt = (n.norm(dataset_norm.denorm(a.to(DEV))).cpu()[:, 0] for a in (p, t))
            per64.append(E.all_metrics(pp.double(), tt.double()))
            per32.append(E.all_metrics(pp, tt))
        for k, v in E.reduce_epoch(per64).items():
            out64[f"{n.stretch_mode}/{names_prefix}{k}"] = v
        for k, v in E.reduce_epoch(per32).items():
            out32[f"{n.stretch_mode}/{names_prefix}{k}"] = v
    return out64, out32


def _check(got: dict, prefix: str, want64: dict, want32: dict):
    assert set(got) >= {f"{prefix}/{k}" for k in want64}
    for k, v in want64.items():
        g = float(got[f"{prefix}/{k}"])
        bar = _bar(want32[k], v) + 1.2e-7 * abs(v)          # compute() returns float32 like the reference's logged values
        print(f"{k}: f64 {v:.9f} collection {g:.9f} |d| {abs(g - v):.2e} bar {bar:.2e}")
        assert abs(g - v) <= bar, (k, g, v)


def test_collection_over_two_batches_and_two_stretch_modes():
    from xmm_superres_denoise.metrics import get_ext_metrics
    from xmm_superres_denoise.transforms import Normalize
    gen = torch.Generator().manual_seed(31)
    batches = [tuple(a.float()[:, None] for a in E.photon_pair((B, 72, 64), gen)) for B in (2, 3)]
    dn, sc = Normalize(1.0, 1.0, "sqrt"), [Normalize(1.0, 1.0, "linear"), Normalize(1.0, 1.0, "sqrt")]
    coll = get_ext_metrics(dn, sc, "test")
    for p, t in batches:
        coll.update(p.to(DEV), t.to(DEV))
    coll.sync()
    got = coll.compute()
    assert set(got) == {f"test/{m}/{n}" for m in ("linear", "sqrt") for n in E.NAMES}
    _check(got, "test", *_expected_epoch(batches, dn, sc))
    coll.reset()
    assert all(st.acc is None for st in coll.states.values())
    # the piq quirk is visible: batches of unequal size do not give the mean over the five images
    with pytest.raises(NotImplementedError, match="single-channel"):
        coll.update(torch.zeros((1, 3, 64, 64), device=DEV), torch.zeros((1, 3, 64, 64), device=DEV))


def test_model_test_step_with_extended_and_input_extended_metrics():
    """SR: the input metrics compare the nearest-upsampled LR image with the target (reference models/model.py:90-105)"""
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.metrics import get_ext_metrics, get_in_ext_metrics
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.transforms import ImageUpsample, Normalize
    from xmm_superres_denoise.utils import Loss
    torch.manual_seed(3)
    dn, sc = Normalize(1.0, 1.0, "linear"), [Normalize(1.0, 1.0, "linear")]
    model = Model(model_cfg("esr_gen", batch_size=2), (48, 56), (96, 112), loss=Loss({"l1": 1.0}),
                  extended_metrics=get_ext_metrics(dn, sc, "test"), in_extended_metrics=get_in_ext_metrics(dn, sc, "test"))
    model.configure_model()
    model.to(DEV)
    gen = torch.Generator().manual_seed(32)
    batches, exp_out, exp_in = [], [], []
    with torch.no_grad():
        for _ in range(2):
            _, hr = (a.float()[:, None] for a in E.photon_pair((2, 96, 112), gen))
            lr = torch.nn.functional.avg_pool2d(hr, 2)
            batches.append((lr, hr))
            exp_out.append((model(lr.to(DEV)).cpu(), hr))
            exp_in.append((ImageUpsample(scale_factor=2)(lr.to(DEV)).cpu(), hr))
            model.test_step((lr.to(DEV), hr.to(DEV)))
        logged = model.on_test_epoch_end()
    assert set(logged) == {"test/loss"} | {f"test/linear/{n}" for n in E.NAMES} | {f"test/linear/in/{n}" for n in E.NAMES}
    _check(logged, "test", *_expected_epoch(exp_out, dn, sc))
    _check(logged, "test", *_expected_epoch(exp_in, dn, sc, "in/"))
    assert model.in_ext_metrics is None and model.ext_metrics is not None       # input metrics are only needed once (reference :135-142)


def test_fit_and_test_with_extended_metrics(tmp_path, capsys):
    from xmm_superres_denoise.metrics.xmm_metric_collection import EXT_NAMES, NAMES
    from xmm_superres_denoise.train import fit, test
    root = dt.make_sim_tree(str(tmp_path / "tree"), n_base=10, n_agn=2, n_bkg=2, lr_exps=(20,), hr_exp=50, hr_mult=1, shape=(60, 52), seed=3)
    ck = str(tmp_path / "run" / "ck.pt")
    os.makedirs(os.path.dirname(ck))
    model, tr, losses = fit("rrdb_denoise", lr_res=320, batch_size=2, dataset_dir=root, hr_exp=50, epochs=1, checkpoint=ck, seed=2,
                            extended_metrics=True)
    out = capsys.readouterr().out
    assert "fsim is the only metric left out" in out and "not computed" not in out
    old = {"test/loss"} | {f"test/linear/{n}" for n in NAMES} | {f"test/linear/in/{n}" for n in NAMES}
    ext = {f"test/linear/{n}" for n in EXT_NAMES} | {f"test/linear/in/{n}" for n in EXT_NAMES}
    assert len(ext) == 10 and set(model.test_logged) == old | ext
    got = test(ck, root, name="rrdb_denoise", lr_res=320, hr_exp=50, batch_size=2, extended_metrics=True)
    out = capsys.readouterr().out
    assert "fsim is the only metric left out" in out and "not computed" not in out and "test/linear/in/haarpsi" in out
    assert set(got) == old | ext
    assert all(np.isfinite(v) for v in got.values()), got
    for k, v in model.test_logged.items():           # test on the best checkpoint gives fit's own test values
        assert abs(float(v) - got[k]) <= 1e-6 * max(1.0, abs(got[k])), k
    plain = test(ck, root, name="rrdb_denoise", lr_res=320, hr_exp=50, batch_size=2)
    out = capsys.readouterr().out
    assert set(plain) == old and "not computed" in out and "fsim" not in out
    for k in old:                                    # the flag changes nothing about what was reported before it existed
        assert plain[k] == got[k], k


def test_two_rank_gloo_collection_reports_the_single_rank_values(tmp_path):
    import ext_metrics_dp_worker as w
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ext_metrics_dp_worker.py"), str(tmp_path)], env=env))
    rcs = [p.wait(timeout=300) for p in procs]
    assert rcs == [0, 0], rcs
    coll = w.collection()
    for p, t in w.batches():
        coll.update(p.to(DEV), t.to(DEV))
    want = w.epoch_values(coll)
    assert len(want) == 10
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert set(z.files) == set(want)
        for k, v in want.items():
            assert abs(float(z[k]) - v) <= 1e-12 * abs(v), (r, k, float(z[k]), v)
