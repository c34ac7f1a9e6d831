"""fsim without a GPU: the plain-torch restatement tests/golden/fsim_torch.py (this project's specification of piq 0.7.x
fsim(chromatic=False); PARITY WITH piq ITSELF IS UNPINNED) against things that do not come from itself, its stored float64 values, and
the host side of the opt-in collection (metrics.XMMFsimCollection, train --fsim)."""
import inspect
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fsim_torch as Fs
import make_golden_fsim as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _pair(shape, seed):
    return Fs.photon_pair(shape, torch.Generator().manual_seed(seed))


# ---- properties of the metric ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 61, 53), (1, 64, 48)])
def test_identical_images_give_one_and_the_value_is_symmetric(shape):
    p, t = _pair(shape, 5)
    assert (Fs.fsim(p, p) - 1).abs().max() < 1e-14
    a, b = Fs.fsim(p, t), Fs.fsim(t, p)
    assert (a - b).abs().max() < 1e-15                 # every term is symmetric in (x, y): products and sums of the same numbers
    assert ((a > 0.5) & (a < 1)).all()
    assert Fs.fsim(p[:, None], t[:, None]).equal(a)     # [B, 1, H, W] is the same batch


def test_joint_horizontal_flip_only_up_to_the_filter_grid():
    """Mirroring both images maps frequency k to -k along that axis.  The radial part of the filters is even in k; the angular part of
    orientation a becomes that of -a, which is the filter of pi - a reflected through the origin, and for a real image that reflection
    only conjugates the response (|eo|, the energy and the median do not see it).  On an ODD axis the grid [-(n-1)/2, (n-1)/2] / (n-1)
    is symmetric, so the value is invariant to rounding: asserted at 1e-10.  On an EVEN axis the grid [-n/2, n/2) / n holds -1/2 but not
    +1/2: the Nyquist column keeps the angle of -1/2 under the flip.  There the low-pass times the largest log-Gabor is < 0.01 of the
    filters' peak (asserted below), one column out of n, so the value moves, but by far less than 1e-3: asserted as such."""
    p, t = _pair((2, 61, 53), 6)
    assert (Fs.fsim(p.flip(-1), t.flip(-1)) - Fs.fsim(p, t)).abs().max() < 1e-10
    p, t = _pair((2, 64, 48), 7)
    d = (Fs.fsim(p.flip(-1), t.flip(-1)) - Fs.fsim(p, t)).abs().max()
    print("even axis: |fsim(flip) - fsim| =", float(d))
    assert d < 1e-3
    f = Fs.construct_filters(64, 48, F64)
    assert f[..., 24].max() < 0.01 * f.max()


@pytest.mark.parametrize("hw", [(61, 53), (64, 48), (8, 6), (3, 3)])
def test_filters_are_zero_at_dc_and_at_most_one(hw):
    f = Fs.construct_filters(*hw, F64)
    assert f.shape == (4, 4) + hw
    assert (f[:, :, 0, 0] == 0).all() and f.max() <= 1 and f.min() >= 0
    if min(hw) > 8:
        assert f.max() > 0.9                              # every scale's radial peak is reached somewhere near its orientation
    radius, theta = Fs.grid(*hw, F64)
    assert radius[0, 0] == 0 and theta[0, 0] == 0
    h, w = hw
    assert abs(radius[h // 2, 0].item() - 0.5) < 1e-15 and abs(radius[0, w // 2].item() - 0.5) < 1e-15        # both grid forms end at 1/2
    lp = Fs.lowpass(*hw, F64)
    assert lp[0, 0] == 1 and abs(lp[h // 2, 0].item() - 1 / (1 + (0.5 / 0.45) ** 30)) < 1e-15


def test_noise_sums_by_parseval():
    """what csrc/fsim.hip computes at plan time instead of transforming the filters: with fe(k) = (f(k) + f(-k)) / 2,
    sum_px g_s g_t = sum_k fe_s fe_t for g = Re(ifft2 f) sqrt(h w)"""
    for h, w in ((61, 53), (64, 48), (9, 12)):
        f = Fs.construct_filters(h, w, F64)
        em_n, an2, aiaj = Fs.noise_constants(f)
        fe = 0.5 * (f + torch.roll(f.flip(-2, -1), (1, 1), (-2, -1)))
        want_an2 = (fe ** 2).sum(dim=[1, 2, 3])
        want_aiaj = sum((fe[:, s] * fe[:, t]).sum(dim=[1, 2]) for s in range(4) for t in range(s + 1, 4))
        assert ((an2 - want_an2).abs() <= 1e-12 * an2).all() and ((aiaj - want_aiaj).abs() <= 1e-12 * aiaj.abs() + 1e-14).all()
        assert (em_n > 0).all()


# ---- the building blocks against explicit loops ------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(53, 61), (8, 6)])
def test_explicit_loop_dft_equals_torch_fft(hw):
    h, w = hw
    x = torch.rand(hw, dtype=F64, generator=torch.Generator().manual_seed(h)) + 1j * torch.rand(hw, dtype=F64, generator=torch.Generator().manual_seed(w))
    a = x.numpy()
    jj, kk = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fwd, inv = np.zeros(hw, complex), np.zeros(hw, complex)
    for u in range(h):
        for v in range(w):
            ph = 2 * np.pi * (((u * jj) % h) / h + ((v * kk) % w) / w)
            fwd[u, v] = (a * np.exp(-1j * ph)).sum()
            inv[u, v] = (a * np.exp(1j * ph)).sum() / (h * w)
    assert np.abs(torch.fft.fft2(x).numpy() - fwd).max() < 1e-11
    assert np.abs(torch.fft.ifft2(x).numpy() - inv).max() < 1e-14


def test_explicit_loop_scharr_and_pooling():
    x = torch.rand((1, 1, 9, 7), dtype=F64, generator=torch.Generator().manual_seed(1))
    a = np.pad(x[0, 0].numpy(), 1)
    k = np.array([[-3.0, 0.0, 3.0], [-10.0, 0.0, 10.0], [-3.0, 0.0, 3.0]]) / 16
    want = np.zeros((9, 7))
    for i in range(9):
        for j in range(7):
            win = a[i:i + 3, j:j + 3]
            want[i, j] = math.sqrt((win * k).sum() ** 2 + (win * k.T).sum() ** 2)
    assert np.abs(Fs.scharr_grad(x)[0, 0].numpy() - want).max() < 1e-15
    for (H, W), ks, hw in (((61, 53), 1, (61, 53)), ((385, 391), 2, (192, 195)), ((417, 403), 2, (208, 201))):
        x = torch.rand((1, 1, H, W), dtype=F64, generator=torch.Generator().manual_seed(H))
        assert Fs.kernel_size(H, W) == ks and Fs.pooled_size(H, W) == hw
        got = Fs.pool(x)[0, 0].numpy()
        assert got.shape == hw                              # the remainder row / column is dropped
        a = x[0, 0].numpy()
        want = np.zeros(hw)
        for i in range(hw[0]):
            for j in range(hw[1]):
                want[i, j] = (255 * a[i * ks:(i + 1) * ks, j * ks:(j + 1) * ks]).sum() / (ks * ks)
        assert np.abs(got - want).max() < 1e-13


def test_kernel_size_rounds_like_python():
    # 127 / 256 = 0.496 -> 0 -> max(1, .); 128 -> 0.5 -> 0 (ties to even) -> 1; 383 -> 1.496 -> 1; 384 -> 1.5 -> 2; 640 -> 2.5 -> 2;
    # 641 -> 2.504 -> 3; 896 -> 3.5 -> 4
    assert [Fs.kernel_size(n, 4096) for n in (127, 128, 383, 384, 640, 641, 896)] == [1, 1, 1, 2, 2, 3, 4]
    assert [Fs.kernel_size(4096, n) for n in (127, 128, 383, 384, 640, 641, 896)] == [1, 1, 1, 2, 2, 3, 4]
    assert Fs.pooled_size(832, 832) == (277, 277) and Fs.pooled_size(640, 640) == (320, 320)


def test_torch_median_takes_the_lower_middle():
    assert torch.median(torch.tensor([4.0, 1.0, 3.0, 2.0])).item() == 2.0
    assert torch.median(torch.tensor([[4.0, 1.0, 3.0, 2.0, 9.0, 0.5]]), dim=-1).values.item() == 2.0
    assert torch.median(torch.tensor([5.0, 1.0, 3.0])).item() == 3.0
    assert math.isnan(torch.median(torch.tensor([5.0, float("nan"), 3.0, 1.0])).item())          # a NaN in the row is what comes out


# ---- stored values -----------------------------------------------------------------------------------------------------
def test_restatement_has_not_drifted_from_the_stored_values():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fsim_cases.npz"))
    assert set(z.files) == {f"{n}/{k}" for n in Fs.CASES for k in ("checksum", "fsim", "num", "pc_max_sum")}
    for name, (H, W, B) in Fs.CASES.items():
        p, t = Fs.case_pair(name)
        assert p.shape == (B, H, W) and p.dtype == torch.float32
        assert np.allclose(z[name + "/checksum"], [p.double().sum().item(), t.double().sum().item()], rtol=1e-12), name
        for k, v in mg.values(p, t).items():
            assert np.allclose(v, z[f"{name}/{k}"], rtol=1e-9, atol=0), (name, k, v, z[f"{name}/{k}"])
        # no case can pass by being NaN on both sides
        assert (z[name + "/pc_max_sum"] > 0).all() and np.isfinite(z[name + "/fsim"]).all(), name
        assert ((z[name + "/fsim"] > 0.5) & (z[name + "/fsim"] < 1)).all(), name


def test_a_pair_without_structure_gives_nan_as_written():
    z = torch.zeros((1, 61, 53), dtype=F64)
    num, den = Fs.fsim_parts(z, z)
    assert den.item() != den.item() or den.item() == 0          # pc is 0 / 0 at every pixel
    assert torch.isnan(Fs.fsim(z, z)).all()
    p, t = _pair((1, 61, 53), 8)
    assert torch.isnan(Fs.fsim(p, z)).all()                      # one all-zero image is enough: its own pc is 0 / 0 at every pixel
    assert torch.isfinite(Fs.fsim(p, t)).all()


# ---- the collection's host side ----------------------------------------------------------------------------------------
def _norms():
    from xmm_superres_denoise.transforms import Normalize
    return Normalize(1.0, 1.0, "sqrt"), [Normalize(1.0, 1.0, "linear"), Normalize(1.0, 1.0, "asinh")]


def test_key_names_signatures_and_notices():
    from xmm_superres_denoise import metrics as M
    from xmm_superres_denoise import train
    from xmm_superres_denoise.models import Model
    dn, sc = _norms()
    for fn in (M.get_fsim_metrics, M.get_in_fsim_metrics):
        assert list(inspect.signature(fn).parameters) == ["dataset_normalizer", "scaling_normalizers", "prefix"]
    assert list(inspect.signature(M.XMMFsimCollection.__init__).parameters)[1:] == ["dataset_normalizer", "scaling_normalizers", "prefix", "input_side"]
    assert inspect.signature(M.XMMFsimCollection.__init__).parameters["input_side"].default is False
    c, ci = M.get_fsim_metrics(dn, sc, "test"), M.get_in_fsim_metrics(dataset_normalizer=dn, scaling_normalizers=sc, prefix="test")
    for coll in (c, ci):
        assert all(hasattr(coll, n) for n in ("update", "sync", "compute", "reset"))
        for st in coll.states.values():
            st.add(torch.tensor([0.25, 0.75], dtype=F64))
    assert set(c.compute()) == {"test/linear/fsim", "test/asinh/fsim"} and set(ci.compute()) == {"test/linear/in/fsim", "test/asinh/in/fsim"}
    assert c.compute()["test/linear/fsim"].dtype == torch.float32 and abs(c.compute()["test/linear/fsim"].item() - 0.25) < 1e-7
    c.reset()
    assert all(st.acc is None for st in c.states.values())
    # the extended collection is what it was: five names, no fsim key
    e = M.get_ext_metrics(dn, sc, "test")
    assert e.names == ("vif_p", "gmsd", "ms_gmsd", "haarpsi", "msdi") and M.EXT_NAMES == e.names
    for fn in (train.fit, train.test):
        assert inspect.signature(fn).parameters["fsim"].default is False
    for n in ("fsim_metrics", "in_fsim_metrics"):
        assert inspect.signature(Model.__init__).parameters[n].default is None
    assert "parity unpinned" in train.FSIM_ON_NOTICE and "fsim" in train.FSIM_ON_NOTICE
    assert "parity unpinned" in train.EXT_AND_FSIM_ON_NOTICE and "fsim" in train.EXT_AND_FSIM_ON_NOTICE
    assert "only metric left out" not in train.EXT_AND_FSIM_ON_NOTICE and "msdi" in train.EXT_AND_FSIM_ON_NOTICE
    # the three pinned texts keep their words
    assert "fsim is the only metric left out" in train.EXT_METRICS_ON_NOTICE and "not computed" in train.EXT_METRICS_NOTICE
    assert "fsim" not in train.EXT_METRICS_NOTICE and M.xmm_metric_collection.FSIM_REFUSAL.startswith("fsim is not on the MI355X engine")
    assert train._notices(False, False) == [train.EXT_METRICS_NOTICE] and train._notices(True, False) == [train.EXT_METRICS_ON_NOTICE]
    assert train._notices(True, True) == [train.EXT_AND_FSIM_ON_NOTICE] and train._notices(False, True) == [train.EXT_METRICS_NOTICE, train.FSIM_ON_NOTICE]


def test_epoch_reduction_is_the_references():
    """the `_Metric` wrapper (metrics/metrics.py:9-27): sum of per-batch MEANS / number of images.  Hand-made per-image values, batches
    of 2 and 3 images."""
    from xmm_superres_denoise.metrics import FsimEpochState
    b1, b2 = torch.tensor([0.10, 0.30], dtype=F64), torch.tensor([0.20, 0.50, 0.80], dtype=F64)
    st = FsimEpochState()
    st.add(b1)
    st.add(b2)
    assert abs(st.compute().item() - (0.2 + 0.5) / 5) < 1e-15              # NOT the mean of the five (0.38)
    assert abs(st.compute().item() - Fs.reduce_epoch([b1, b2])) < 1e-15
    st.sync()             # no process group: a no-op
    assert abs(st.compute().item() - 0.14) < 1e-15


def _uneven_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from xmm_superres_denoise.metrics import FsimEpochState
    st = FsimEpochState()
    if rank == 0:       # rank 1's test shard is empty: it must still enter the collective
        st.add(torch.tensor([0.10, 0.30], dtype=F64))
        st.add(torch.tensor([0.20, 0.50, 0.80], dtype=F64))
    st.sync()
    both = FsimEpochState()
    both.add(torch.tensor([0.4, 0.6] if rank == 0 else [0.1, 0.2, 0.9], dtype=F64))
    both.sync()
    empty = FsimEpochState()
    empty.sync()        # nobody saw a batch: the collective still matches and the state stays empty
    ret[rank] = (float(st.compute()), float(both.compute()), empty.acc is None)
    dist.destroy_process_group()


def test_sync_over_two_gloo_ranks_with_an_empty_rank():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_uneven_worker, args=(2, port, ret), nprocs=2, join=True)
    assert ret[0] == ret[1]
    one, both, empty = ret[0]
    assert abs(one - 0.14) < 1e-15 and abs(both - (0.5 + 0.4) / 5) < 1e-15 and empty


@pytest.mark.parametrize("flags", [(), ("--fsim",), ("--fsim", "--extended-metrics")])
def test_cli_fsim_reaches_test_and_fit(monkeypatch, flags):
    from xmm_superres_denoise import train
    seen = {}
    monkeypatch.setattr(train, "test", lambda *a, **k: seen.update(k, args=a))
    monkeypatch.setattr(sys, "argv", ["train.py", "test", "--model", "hat", "--checkpoint", "c.ckpt", "--dataset-dir", "d", *flags])
    train.main()
    assert seen["fsim"] is ("--fsim" in flags) and seen["extended_metrics"] is ("--extended-metrics" in flags) and seen["name"] == "hat"
    seen.clear()
    monkeypatch.setattr(train, "fit", lambda *a, **k: seen.update(k, args=a))
    monkeypatch.setattr(sys, "argv", ["train.py", "fit", "--dataset-dir", "d", *flags])
    train.main()
    assert seen["fsim"] is ("--fsim" in flags) and seen["extended_metrics"] is ("--extended-metrics" in flags)


def test_the_extended_collection_still_refuses_fsim():
    from xmm_superres_denoise.metrics import XMMExtMetricCollection, get_fsim_metrics
    from xmm_superres_denoise.metrics.xmm_metric_collection import FSIM_REFUSAL
    dn, sc = _norms()
    with pytest.raises(NotImplementedError, match="fsim is not on the MI355X engine"):
        XMMExtMetricCollection(("fsim",), dn, sc, "test")
    with pytest.raises(NotImplementedError, match="in/fsim"):
        XMMExtMetricCollection(("in/fsim",), dn, sc, "test")
    assert "278 = 2 * 139" in FSIM_REFUSAL
    c = get_fsim_metrics(dn, sc, "test")
    for shape in ((2, 3, 64, 64), (2, 64, 64)):
        with pytest.raises(NotImplementedError, match="single-channel"):
            c.update(torch.zeros(shape), torch.zeros(shape))
