"""fsim on the MI355X (csrc/fsim.hip, xsd_fsim_eval): piq 0.7.x fsim(chromatic=False), the sixth extended test metric, opt-in.

The comparator is the plain-torch restatement tests/golden/fsim_torch.py on the CPU -- this project's specification of the metric,
restated from piq's published code.  PARITY WITH piq ITSELF IS UNPINNED (piq is not available here).

Accuracy rule per image:  |engine - f64| <= max(2 * |f32 - f64|, 5e-6 * max(1, |f64|)),  f32 / f64 = the restatement in the two dtypes on
the same fp32-representable inputs (the rule of test_hip_ext_metrics.py).  The transform alone: max |err| / max |X| against torch.fft in
float64 at most twice what torch.fft in float32 on the CPU shows (the project's 2x convention).  The selection alone: bitwise."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_tree as dt
import fsim_torch as Fs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_cache = {}


def _case(size):
    """the seeded photon-like pairs of the size (fp32), and the restatement's values in float64 and float32"""
    if size not in _cache:
        p, t = Fs.case_pair(size)
        _cache[size] = (p, t, Fs.fsim(p.double(), t.double()), Fs.fsim(p, t))
    return _cache[size]


def _bar(f32, f64):
    return max(2 * abs(f32 - f64), 5e-6 * max(1.0, abs(f64)))


@pytest.fixture(scope="module")
def engine():
    from xmm_superres_denoise.engine import FsimEngine
    with torch.cuda.device(DEV):
        return FsimEngine()


@pytest.mark.parametrize("shape", [(3, 53, 61), (2, 48, 64), (1, 201, 208), (1, 277, 277)])
def test_dft2_alone(engine, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.complex(torch.randn(shape, generator=g), torch.randn(shape, generator=g))
    xd = torch.view_as_real(x).contiguous().to(DEV)
    for inverse, fn in ((False, torch.fft.fft2), (True, torch.fft.ifft2)):
        want = fn(x.to(torch.complex128))
        scale = want.abs().max().item()
        ref32 = (fn(x).to(torch.complex128) - want).abs().max().item() / scale
        out = torch.full(xd.shape, float("nan"), device=DEV)          # sentinel: every element must be overwritten
        got = engine.dft2(xd, inverse=inverse, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.isfinite(out).all()
        err = (torch.view_as_complex(out.cpu()).to(torch.complex128) - want).abs().max().item() / scale
        print(f"dft2 {shape} {'inverse' if inverse else 'forward'}: engine {err:.3e} torch.fft fp32 {ref32:.3e} ratio {err / ref32:.3f}")
        assert err <= 2 * ref32, (shape, inverse, err, ref32)
    # round trip
    back = engine.dft2(engine.dft2(xd), inverse=True)
    scale = x.abs().max().item()
    ref32 = (torch.fft.ifft2(torch.fft.fft2(x)) - x).abs().max().item() / scale
    err = (torch.view_as_complex(back.cpu()) - x).abs().max().item() / scale
    print(f"dft2 {shape} round trip: engine {err:.3e} torch.fft fp32 {ref32:.3e}")
    assert err <= 2 * ref32, (shape, err, ref32)


def test_median_alone():
    from xmm_superres_denoise.engine import fsim_median
    g = torch.Generator().manual_seed(9)
    for n in (53 * 61, 48 * 64):                       # odd and even counts
        rows = torch.rand((7, n), generator=g) ** 2
        rows[1] = 0.375                                # all equal
        rows[2, : n // 2] = 0.0                        # half zeros: for the even count the lower middle is a zero, the upper one is not
        rows[2, n // 2:] += 0.5
        rows[3] = torch.randint(0, 5, (n,), generator=g).float() / 4          # many duplicates
        rows[4] = rows[4] * 1e-30                      # tiny values, some denormal
        rows[5, 1234] = float("nan")
        rows[6] = rows[6] * 3e38                       # the top of the exponent range
        out = torch.full((7,), -1.0, device=DEV)
        got = fsim_median(rows.to(DEV), out=out).cpu()
        want = torch.median(rows, dim=-1).values
        keep = [0, 1, 2, 3, 4, 6]
        assert torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32)), (n, got, want)
        # a row that holds a NaN gives NaN, as torch.median does; its neighbours are untouched (checked bitwise above)
        assert torch.isnan(got[5]) and torch.isnan(want[5])
        assert got[2] == (0.0 if n % 2 == 0 else want[2])
    one = fsim_median(torch.tensor([[2.5]], device=DEV))
    assert one.item() == 2.5


@pytest.mark.parametrize("size,B", [("61x53", 1), ("61x53", 4), ("64x48", 1), ("64x48", 4), ("417x403", 1), ("417x403", 4), ("832x832", 1)])
def test_accuracy_against_the_float64_restatement(engine, size, B):
    """measured (profiles/r13_fsim_gputest.log): worst |engine - f64| / bar per size"""
    p, t, f64, f32 = _case(size)
    got = engine.eval(p[:B].to(DEV), t[:B].to(DEV)).cpu()
    misses = []
    for b in range(B):
        g, v64, v32 = got[b].item(), f64[b].item(), float(f32[b].item())
        bar = _bar(v32, v64)
        print(f"{size} B={B} image {b} f64 {v64:.12f} engine {g:.12f} |engine-f64| {abs(g - v64):.2e} |f32-f64| {abs(v32 - v64):.2e} "
              f"bar {bar:.2e} err/bar {abs(g - v64) / bar:.3f}")
        if not abs(g - v64) <= bar:
            misses.append((b, g, v64, v32))
    assert not misses, misses


def test_batch_independence_and_determinism_bitwise(engine):
    from xmm_superres_denoise.engine import FsimEngine
    for size in ("61x53", "64x48"):
        p, t = (a.to(DEV) for a in _case(size)[:2])
        a = engine.eval(p, t)
        assert torch.equal(a, engine.eval(p, t))
        singles = torch.cat([engine.eval(p[i:i + 1].contiguous(), t[i:i + 1].contiguous()) for i in range(4)])
        assert torch.equal(a, singles)
        assert torch.equal(a, engine.eval(p[:, None], t[:, None]))              # a [B, 1, H, W] tensor is the same batch
        b = FsimEngine().eval(p.flip(0).contiguous(), t.flip(0).contiguous())   # another object, another position, other neighbours
        assert torch.equal(a, b.flip(0))
        assert torch.isfinite(a).all()


@pytest.mark.parametrize("where", ["preds", "target"])
def test_nan_pixel_stays_in_its_image(engine, where):
    p, t, _, _ = _case("61x53")
    clean = engine.eval(p.to(DEV), t.to(DEV))
    p, t = p.clone(), t.clone()
    (p if where == "preds" else t)[2, 30, 17] = float("nan")
    got = engine.eval(p.to(DEV), t.to(DEV))
    assert torch.equal(got[[0, 1, 3]], clean[[0, 1, 3]]) and torch.isfinite(clean).all()
    want = Fs.fsim(p.double(), t.double())
    assert not torch.isfinite(want[2]) and not torch.isfinite(got[2])


def test_constant_pair_gives_nan_as_written(engine):
    """The constant pair whose sum of pc_max is exactly 0 in any arithmetic is the all-zero one (every response is an exact zero; a
    non-zero constant leaves rounding residue off DC, so its value is rounding noise over rounding noise: unspecified, finite or NaN,
    in the restatement and in the engine alike, and not asserted)."""
    p, t, f64, _ = _case("61x53")
    p, t = p.clone(), t.clone()
    p[1] = 0.0
    t[1] = 0.0
    want = Fs.fsim(p.double(), t.double())
    got = engine.eval(p.to(DEV), t.to(DEV)).cpu()
    assert torch.isnan(want[1]) and torch.isnan(got[1])
    for b in (0, 2, 3):
        assert abs(got[b].item() - f64[b].item()) <= 5e-6 and torch.isfinite(got[b])


def test_refusals(engine):
    from xmm_superres_denoise.engine import XsdError, _lib, fsim_median
    z = torch.zeros((1, 1, 64, 64), device=DEV)
    with pytest.raises(XsdError, match="C must be 1"):
        engine.eval(torch.zeros((1, 3, 64, 64), device=DEV), torch.zeros((1, 3, 64, 64), device=DEV))
    with pytest.raises(XsdError, match="3..1024 pixels a side"):
        engine.eval(torch.zeros((1, 1, 2, 2), device=DEV), torch.zeros((1, 1, 2, 2), device=DEV))
    with pytest.raises(XsdError, match="3..1024 pixels a side"):
        engine.eval(torch.zeros((2, 64, 2), device=DEV), torch.zeros((2, 64, 2), device=DEV))
    engine.eval(torch.zeros((1, 3, 3), device=DEV), torch.zeros((1, 3, 3), device=DEV))       # the smallest size is taken
    with pytest.raises(XsdError, match="shape mismatch"):
        engine.eval(z, torch.zeros((1, 1, 64, 65), device=DEV))
    with pytest.raises(XsdError, match="no CPU fallback"):
        engine.eval(z.cpu(), z.cpu())
    with pytest.raises(XsdError, match="float32"):
        engine.eval(z.double(), z.double())
    with pytest.raises(XsdError, match="contiguous"):
        engine.eval(torch.zeros((1, 1, 64, 128), device=DEV)[..., ::2], z)
    with pytest.raises(XsdError, match=r"\[B,H,W\]"):
        engine.eval(z[0, 0], z[0, 0])
    with pytest.raises(XsdError, match="3..1024"):
        engine.dft2(torch.zeros((1, 2, 8, 2), device=DEV))
    with pytest.raises(XsdError, match="re, im"):
        engine.dft2(torch.zeros((1, 8, 8), device=DEV))
    with pytest.raises(XsdError, match="no CPU fallback"):
        fsim_median(torch.zeros((1, 8)))
    L = _lib.load()
    out = torch.zeros((1,), dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert L.xsd_fsim_eval(engine.h, z.data_ptr(), z.data_ptr(), out.data_ptr(), 0, 1, 64, 64, stream) == -1
    assert b"B must be" in L.xsd_last_error()
    for args in ((None, z.data_ptr(), z.data_ptr(), out.data_ptr()), (engine.h, None, z.data_ptr(), out.data_ptr()),
                 (engine.h, z.data_ptr(), None, out.data_ptr()), (engine.h, z.data_ptr(), z.data_ptr(), None)):
        assert L.xsd_fsim_eval(*args, 1, 1, 64, 64, stream) == -1
        assert b"null pointer" in L.xsd_last_error()
    assert L.xsd_fsim_create(None) == -1
    L.xsd_fsim_destroy(None)
    torch.cuda.synchronize()


def test_two_sizes_alternate(engine):
    from xmm_superres_denoise.engine import FsimEngine
    cases = [tuple(a.to(DEV) for a in _case(size)[:2]) for size in ("64x48", "61x53")]
    fresh = [FsimEngine().eval(p, t) for p, t in cases]
    one = FsimEngine()
    for _ in range(3):
        for (p, t), want in zip(cases, fresh):
            assert torch.equal(one.eval(p, t), want)
    # more sizes than the handle keeps plans for: the evicted one is rebuilt to the same bits
    for n in (40, 41, 42, 43):
        z = torch.rand((1, n, n + 3), device=DEV)
        one.eval(z, z)
    assert torch.equal(one.eval(*cases[0]), fresh[0])


def _expected_epoch(batches, dataset_norm, scaling, name="fsim"):
    """the collection's values from the restatement: per batch denorm -> renorm on the device (the engine's own stretch kernels, tested
    elsewhere), the restatement in float64 / float32 on the CPU, the reference's epoch reduction"""
    out64, out32 = {}, {}
    for n in scaling:
        per64, per32 = [], []
        for p, t in batches:
            pp, tt = (n.norm(dataset_norm.denorm(a.to(DEV))).cpu()[:, 0] for a in (p, t))
            per64.append(Fs.fsim(pp.double(), tt.double()))
            per32.append(Fs.fsim(pp, tt))
        out64[f"{n.stretch_mode}/{name}"] = Fs.reduce_epoch(per64)
        out32[f"{n.stretch_mode}/{name}"] = Fs.reduce_epoch(per32)
    return out64, out32


def _check(got: dict, prefix: str, want64: dict, want32: dict):
    assert set(got) >= {f"{prefix}/{k}" for k in want64}
    for k, v in want64.items():
        g = float(got[f"{prefix}/{k}"])
        bar = _bar(want32[k], v) + 1.2e-7 * abs(v)          # compute() returns float32 like the reference's logged values
        print(f"{k}: f64 {v:.9f} collection {g:.9f} |d| {abs(g - v):.2e} bar {bar:.2e}")
        assert abs(g - v) <= bar, (k, g, v)


def test_collection_two_batches_two_stretch_modes():
    from xmm_superres_denoise.metrics import get_fsim_metrics
    from xmm_superres_denoise.transforms import Normalize
    gen = torch.Generator().manual_seed(31)
    batches = [tuple(a.float()[:, None] for a in Fs.photon_pair((B, 72, 64), gen)) for B in (2, 3)]
    dn, sc = Normalize(1.0, 1.0, "sqrt"), [Normalize(1.0, 1.0, "linear"), Normalize(1.0, 1.0, "sqrt")]
    coll = get_fsim_metrics(dn, sc, "test")
    for p, t in batches:
        coll.update(p.to(DEV), t.to(DEV))
    coll.sync()
    got = coll.compute()
    assert set(got) == {"test/linear/fsim", "test/sqrt/fsim"}
    w64, w32 = _expected_epoch(batches, dn, sc)
    _check(got, "test", w64, w32)
    # the `_Metric` quirk is visible: batches of unequal size do not give the mean over the five images
    coll.reset()
    assert all(st.acc is None for st in coll.states.values())
    with pytest.raises(NotImplementedError, match="single-channel"):
        coll.update(torch.zeros((1, 3, 64, 64), device=DEV), torch.zeros((1, 3, 64, 64), device=DEV))


def test_model_test_step_with_fsim():
    """SR: the input side compares the nearest-upsampled LR image with the target (reference models/model.py:90-105)"""
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.metrics import get_fsim_metrics, get_in_fsim_metrics
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.transforms import ImageUpsample, Normalize
    from xmm_superres_denoise.utils import Loss
    torch.manual_seed(3)
    dn, sc = Normalize(1.0, 1.0, "linear"), [Normalize(1.0, 1.0, "linear")]
    model = Model(model_cfg("esr_gen", batch_size=2), (48, 56), (96, 112), loss=Loss({"l1": 1.0}),
                  fsim_metrics=get_fsim_metrics(dn, sc, "test"), in_fsim_metrics=get_in_fsim_metrics(dn, sc, "test"))
    assert model.ext_metrics is None and model.in_ext_metrics is None
    model.configure_model()
    model.to(DEV)
    gen = torch.Generator().manual_seed(32)
    exp_out, exp_in = [], []
    with torch.no_grad():
        for _ in range(2):
            _, hr = (a.float()[:, None] for a in Fs.photon_pair((2, 96, 112), gen))
            lr = torch.nn.functional.avg_pool2d(hr, 2)
            exp_out.append((model(lr.to(DEV)).cpu(), hr))
            exp_in.append((ImageUpsample(scale_factor=2)(lr.to(DEV)).cpu(), hr))
            model.test_step((lr.to(DEV), hr.to(DEV)))
        logged = model.on_test_epoch_end()
    assert set(logged) == {"test/loss", "test/linear/fsim", "test/linear/in/fsim"}
    _check(logged, "test", *_expected_epoch(exp_out, dn, sc))
    _check(logged, "test", *_expected_epoch(exp_in, dn, sc, "in/fsim"))
    assert model.in_fsim_metrics is None and model.fsim_metrics is not None       # input metrics are only needed once (reference :135-142)


def test_fit_and_test_with_fsim(tmp_path, capsys):
    from xmm_superres_denoise import train
    from xmm_superres_denoise.metrics.xmm_metric_collection import EXT_NAMES, NAMES
    root = dt.make_sim_tree(str(tmp_path / "tree"), n_base=10, n_agn=2, n_bkg=2, lr_exps=(20,), hr_exp=50, hr_mult=1, shape=(60, 52), seed=3)
    ck = str(tmp_path / "run" / "ck.pt")
    os.makedirs(os.path.dirname(ck))
    model, tr, losses = train.fit("rrdb_denoise", lr_res=320, batch_size=2, dataset_dir=root, hr_exp=50, epochs=1, checkpoint=ck, seed=2, fsim=True)
    out = capsys.readouterr().out
    assert train.FSIM_ON_NOTICE in out and "not computed" in out and "only metric left out" not in out
    old = {"test/loss"} | {f"test/linear/{n}" for n in NAMES} | {f"test/linear/in/{n}" for n in NAMES}
    new = {"test/linear/fsim", "test/linear/in/fsim"}
    assert set(model.test_logged) == old | new
    plain = train.test(ck, root, name="rrdb_denoise", lr_res=320, hr_exp=50, batch_size=2)
    out = capsys.readouterr().out
    assert set(plain) == old and "not computed" in out and "fsim" not in out          # without the flag: no new word
    got = train.test(ck, root, name="rrdb_denoise", lr_res=320, hr_exp=50, batch_size=2, fsim=True)
    out = capsys.readouterr().out
    assert train.FSIM_ON_NOTICE in out and "parity unpinned" in out and "test/linear/in/fsim" in out
    assert set(got) == old | new and all(np.isfinite(v) for v in got.values()), got
    assert 0 < got["test/linear/fsim"] <= 1 and 0 < got["test/linear/in/fsim"] <= 1
    for k in old:                                    # the flag changes nothing about what was reported before it existed
        assert plain[k] == got[k], k
    for k, v in model.test_logged.items():           # test on the best checkpoint gives fit's own test values
        assert abs(float(v) - got[k]) <= 1e-6 * max(1.0, abs(got[k])), k
    both = train.test(ck, root, name="rrdb_denoise", lr_res=320, hr_exp=50, batch_size=2, fsim=True, extended_metrics=True)
    out = capsys.readouterr().out
    assert train.EXT_AND_FSIM_ON_NOTICE in out and "only metric left out" not in out and "not computed" not in out
    ext = {f"test/linear/{n}" for n in EXT_NAMES} | {f"test/linear/in/{n}" for n in EXT_NAMES}
    assert set(both) == old | new | ext
    for k in old | new:
        assert both[k] == got[k], k


def test_two_rank_gloo_collection_reports_the_single_rank_values(tmp_path):
    import fsim_dp_worker as w
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "fsim_dp_worker.py"), str(tmp_path)], env=env))
    rcs = [p.wait(timeout=300) for p in procs]
    assert rcs == [0, 0], rcs
    coll = w.collection()
    for p, t in w.batches():
        coll.update(p.to(DEV), t.to(DEV))
    want = w.epoch_values(coll)
    assert len(want) == 2
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert set(z.files) == set(want)
        for k, v in want.items():
            assert abs(float(z[k]) - v) <= 1e-12 * abs(v), (r, k, float(z[k]), v)
