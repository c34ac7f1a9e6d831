"""The dataset feed on the MI355X: xsd_compose_batch against xsd_compose_input, the reference's own composed tensors
(tests/golden/dataset_sim.npz, make_golden_dataset.py), batch independence, a dataset-fed fit + test, and a 2-rank fit."""
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_tree as dt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "dataset_sim.npz"))
DEV = "cuda:0"


@pytest.mark.parametrize("is_int32", [True, False])
@pytest.mark.parametrize("big_endian", [True, False])
def test_compose_batch_equals_compose_input_bitwise(is_int32, big_endian):
    from xmm_superres_denoise.engine import compose_batch, compose_input
    g = np.random.default_rng(7 + 2 * is_int32 + big_endian)
    H, W, n_slots = 37, 29, 6
    vals = g.poisson(3.0, (n_slots, H, W)).astype(np.int32) if is_int32 else (g.random((n_slots, H, W)) * 5e-3).astype(np.float32)
    words = vals.view(np.uint32)
    if big_endian:
        words = words.byteswap()
    pool = torch.from_numpy(words.view(np.int32).reshape(n_slots, H * W).copy()).to(DEV)
    stacked = torch.from_numpy(words.view(np.int32 if is_int32 else np.float32).copy()).to(DEV)
    mask = torch.from_numpy((g.random((H, W)) > 0.3).astype(np.uint8)).to(DEV)
    img, agn, bkg = [4, 0, 4, 2], [1, -1, 5, 3], [2, 3, -1, 0]
    for m in (None, mask):
        for up, res in ((1, 48), (1, 32), (2, 80)):
            for stretch, mx in (("linear", None), ("linear", 3.0), ("sqrt", 3.0), ("asinh", 2e-3), ("log", 4e-3)):
                mv = None if mx is None else (mx if is_int32 else mx * 1e-3)
                got = compose_batch(pool, img, agn, bkg, m, H, W, res, mv, stretch, up, is_int32, big_endian)
                for b in range(4):
                    ref = compose_input(stacked[img[b]][None], stacked[agn[b]][None] if agn[b] >= 0 else None,
                                        stacked[bkg[b]][None] if bkg[b] >= 0 else None, m, res, mv, stretch, up, big_endian)
                    assert torch.equal(got[b].view(torch.int32), ref[0].view(torch.int32)), (m is None, up, res, stretch, b)
    # no agn / bkg array at all = absent for every sample
    got = compose_batch(pool, img, None, None, mask, H, W, 48, None, "linear", 1, is_int32, big_endian)
    ref = compose_input(stacked[img], None, None, mask, 48, None, "linear", 1, big_endian)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_compose_batch_refuses_an_out_of_range_index():
    from xmm_superres_denoise.engine import XsdError, compose_batch
    pool = torch.zeros((3, 20), dtype=torch.int32, device=DEV)
    with pytest.raises(XsdError, match="sample 1: img slot 3 outside the pool's 3 slots"):
        compose_batch(pool, [0, 3], None, None, None, 4, 5, 8, None)
    with pytest.raises(XsdError, match="sample 0: bkg slot -2"):
        compose_batch(pool, [0, 1], [0, 0], [-2, 0], None, 4, 5, 8, None)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def golden_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("golden_tree")
    dt.golden_tree(str(root), Z)
    mz = np.load(os.path.join(ROOT, "tests", "golden", "example_data.npz"))
    masks = {w: dt.write_fits(str(root / "masks" / f"mask_{w}.fits"), dt.unpack_mask(mz, w), bitpix=8) for w in ("1x", "2x")}
    return root, masks


def _ds(root, kind, masks=None, exps=(20,)):
    from xmm_superres_denoise.data.dataset import XmmDataset
    from xmm_superres_denoise.train import dataset_cfg
    dn = kind == "dn"
    cfg = dataset_cfg(str(root), name="rrdb_denoise" if dn else "esr_gen", lr_exps=exps, hr_exp=50 if dn else 100,
                      lr_det_mask=masks["1x"] if masks else None, hr_det_mask=(masks["1x" if dn else "2x"] if masks else None))
    return XmmDataset(cfg).build_pool(device=DEV)


def test_golden_combinations_match_the_reference_sha256(golden_root):
    from xmm_superres_denoise.engine import compose_batch
    root, masks = golden_root
    for i, row in enumerate(Z["combos"]):
        lr_img, lr_agn, lr_bkg, hr_img, hr_agn, kind, _, hm, hres, masked = [str(c) for c in row]
        d = _ds(root, kind, masks if masked == "1" else None)
        lslot = [d.lr_pool.files.index(root / p) for p in (lr_img, lr_agn, lr_bkg)]
        hslot = [d.hr_pool.files.index(root / p) for p in (hr_img, hr_agn)]
        c = d.config
        lr = compose_batch(d.lr_pool.words, lslot[:1], lslot[1:2], lslot[2:], d.lr_mask, *d.lr_pool.shape, 416, c.lr.clamp_max, "sqrt")
        hr = compose_batch(d.hr_pool.words, hslot[:1], hslot[1:], None, d.hr_mask, *d.hr_pool.shape, int(hres), c.hr.clamp_max, "sqrt")
        for what, t in (("lr", lr), ("hr", hr)):
            a = t[0].cpu().numpy()
            assert hashlib.sha256(a.tobytes()).hexdigest() == str(Z[f"combo{i}_{what}_sha256"]), (i, what)
            assert a.astype(np.float64).sum() == Z[f"combo{i}_sums"][0 if what == "lr" else 1]


def test_batch_of_four_equals_four_batches_of_one(golden_root):
    root, masks = golden_root
    for kind in ("dn", "sr"):
        d = _ds(root, kind, masks, exps=(20, 50))
        idx = d.samples_of([1, 0])
        lr, hr = d.batch(idx, epoch=3)
        hs = 416 if kind == "dn" else 832
        assert lr.shape == (4, 1, 416, 416) and hr.shape == (4, 1, hs, hs)
        for i, s in enumerate(idx):
            l1, h1 = d.batch([s], epoch=3)
            assert torch.equal(l1[0], lr[i]) and torch.equal(h1[0], hr[i])
        # the choices depend on (seed, epoch, sample): another epoch may pick other files, the same epoch the same ones
        assert d.file_names(idx, 3) == d.file_names(idx[::-1], 3)[::-1]


def test_fit_two_epochs_keeps_the_best_checkpoint_and_tests_it(tmp_path, capsys):
    from xmm_superres_denoise.train import fit, test
    root = dt.make_sim_tree(str(tmp_path / "tree"), n_base=10, n_agn=2, n_bkg=2, lr_exps=(20,), hr_exp=50, hr_mult=1, shape=(60, 52), seed=3)
    ck = str(tmp_path / "run" / "ck.pt")
    os.makedirs(os.path.dirname(ck))
    model, tr, losses = fit("rrdb_denoise", lr_res=320, batch_size=2, dataset_dir=root, hr_exp=50, epochs=2, checkpoint=ck, seed=2)
    out = capsys.readouterr().out
    vals = [h["val/loss"] for h in model.history]
    assert len(vals) == 2 and os.path.exists(ck) and os.path.exists(str(tmp_path / "run" / "sim_dataset_sim_img_splits.json"))
    assert "epoch 0: train/loss" in out and "epoch 1: train/loss" in out and "val/loss" in out
    ckd = torch.load(ck, weights_only=True)
    assert ckd["epoch"] == int(np.argmin(vals))
    got = test(ck, root, name="rrdb_denoise", lr_res=320, hr_exp=50, batch_size=2)
    out = capsys.readouterr().out
    from xmm_superres_denoise.metrics.xmm_metric_collection import NAMES
    want = {"test/loss"} | {f"test/linear/{n}" for n in NAMES} | {f"test/linear/in/{n}" for n in NAMES}
    assert set(got) == want, set(got) ^ want
    assert all(np.isfinite(v) for v in got.values())
    assert "get_ext_metrics" in out and "piq" in out and "not computed" in out
    # test on the best checkpoint gives fit's own test values
    for k, v in model.test_logged.items():
        assert abs(float(v) - got[k]) <= 1e-6 * max(1.0, abs(got[k])), k


def test_two_rank_gloo_fit_ends_with_identical_replicas(tmp_path):
    root = dt.make_sim_tree(str(tmp_path / "tree"), n_base=10, n_agn=1, n_bkg=1, lr_exps=(20,), hr_exp=50, hr_mult=1, shape=(40, 36), seed=4)
    out = tmp_path / "out"
    out.mkdir()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   XSD_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dataset_dp_worker.py"), root, str(out), "320"], env=env))
    rcs = [p.wait(timeout=300) for p in procs]
    assert rcs == [0, 0], rcs
    a, b = np.load(out / "rank0.npz"), np.load(out / "rank1.npz")
    assert np.array_equal(a["params"], b["params"]) and np.array_equal(a["losses"], b["losses"]) and len(a["losses"]) == 2
