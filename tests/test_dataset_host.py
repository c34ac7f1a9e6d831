"""CPU checks of the dataset feed (xmm_superres_denoise/data/dataset.py, datamodule.py): discovery and matching against what
the reference's own code found on the recorded tree (tests/golden/dataset_sim.npz, make_golden_dataset.py), seeded splits,
rank shards, and the refusals that name what they refuse."""
import json
import os

import numpy as np
import pytest

import dataset_tree as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "dataset_sim.npz"))


def _cfg(root, exps=(20,), hr_exp=100, hr_res=832, **kw):
    from xmm_superres_denoise.train import dataset_cfg
    name = "esr_gen" if hr_res == 832 else "rrdb_denoise"
    return dataset_cfg(str(root), lr_exps=exps, hr_exp=hr_exp, name=name, **kw)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("golden_tree")
    dt.golden_tree(str(root), Z)
    return root


@pytest.mark.parametrize("tag,exps", [("e20", (20,)), ("e20_50", (20, 50))])
def test_discovery_and_matching_reproduce_the_reference(tree, tag, exps):
    from xmm_superres_denoise.data.dataset import XmmDataset
    d = XmmDataset(_cfg(tree, exps))
    assert d.base_name_count == int(Z[f"{tag}_base_name_count"][0])
    assert d.dataset_size == int(Z[f"{tag}_dataset_size"][0])
    assert d.base_names == [str(s) for s in Z[f"{tag}_base_names"]]
    assert [[";".join(c) for c in row] for row in d.lr_img_files.names()] == [[str(c) for c in row] for row in Z[f"{tag}_lr_files"]]
    assert [";".join(row[0]) for row in d.hr_img_files.names()] == [str(c) for c in Z[f"{tag}_hr_files"]]
    assert d.base_agn_count == int(Z[f"{tag}_agn_count"][0])
    assert len(d) == d.base_name_count * len(exps) * 1 * 1


def test_real_type_matching_reproduces_the_reference(tmp_path):
    from pathlib import Path
    from xmm_superres_denoise.data.tools import find_img_dirs, find_img_files, match_file_list
    for e in (20, 50):
        os.makedirs(tmp_path / f"{e}ks")
        for n in Z[f"real_names_{e}"]:
            (tmp_path / f"{e}ks" / str(n)).touch()
    lr = find_img_files(find_img_dirs(Path(tmp_path), [20], ""))
    hr = find_img_files(find_img_dirs(Path(tmp_path), [50], ""))
    lr_t, hr_t, n = match_file_list(lr, hr, "_image_split_")
    assert lr_t.index == [str(s) for s in Z["real_base_names"]] and n == len(Z["real_base_names"])
    assert [";".join(r[0]) for r in lr_t.names()] == [str(s) for s in Z["real_lr_files"]]
    assert [";".join(r[0]) for r in hr_t.names()] == [str(s) for s in Z["real_hr_files"]]


def test_index_map_and_sample_enumeration(tree):
    from xmm_superres_denoise.data.dataset import XmmDataset
    d1 = XmmDataset(_cfg(tree, (20,)))
    # one exposure, agn = bkg = 1: the reference's load_sample map (base = idx % base_name_count) and its split indices
    b, e, r = d1.decode(np.arange(d1.dataset_size))
    assert list(b) == list(np.arange(d1.dataset_size) % d1.base_name_count) and not e.any() and not r.any()
    assert list(d1.samples_of([1, 0])) == [1, 0]
    d2 = XmmDataset(_cfg(tree, (20, 50)), seed=0)
    sm = d2.samples_of([0, 1])
    b, e, r = d2.decode(sm)
    assert sorted(zip(b.tolist(), e.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]     # every (base, exposure) pair
    with pytest.raises(IndexError, match="outside the dataset"):
        d2.decode([d2.dataset_size])


def test_splits_are_seeded_disjoint_complete_and_reused(tmp_path):
    from xmm_superres_denoise.data.datamodule import load_or_make_splits, make_splits, split_bases
    from xmm_superres_denoise.data.dataset import XmmDataset
    root = dt.make_sim_tree(str(tmp_path / "t"), n_base=10, n_agn=1, n_bkg=1, shape=(4, 5), hr_mult=2, hr_exp=100)
    d = XmmDataset(_cfg(root))
    s1, s2 = make_splits(d, seed=3), make_splits(d, seed=3)
    assert s1 == s2 and make_splits(d, seed=4) != s1
    assert [len(s1[k]) for k in ("train", "val", "test")] == [8, 1, 1]
    allnames = s1["train"] + s1["val"] + s1["test"]
    assert sorted(allnames) == sorted(d.base_names) and len(set(allnames)) == 10
    p = str(tmp_path / "run" / "splits.json")
    got = load_or_make_splits(d, p, seed=3)
    assert got == s1 and json.load(open(p))["train"] == s1["train"]
    # the file wins over the seed afterwards
    assert load_or_make_splits(d, p, seed=99) == s1
    assert sorted(split_bases(d, s1["val"], "val")) == sorted(d.base_names.index(n) for n in s1["val"])


@pytest.mark.parametrize("world", [2, 8])
def test_rank_shards_cover_the_epoch(world):
    from xmm_superres_denoise.data.datamodule import shard
    n = 21
    for epoch in (0, 1):
        parts = [shard(n, epoch, r, world, shuffle=True, seed=5) for r in range(world)]
        assert len({len(p) for p in parts}) == 1 and len(parts[0]) == -(-n // world)
        allpos = np.concatenate(parts)
        assert set(allpos.tolist()) == set(range(n))
        assert len(allpos) - len(set(allpos.tolist())) == -(-n // world) * world - n     # only the wrap-around padding repeats
    assert not np.array_equal(shard(n, 0, 0, world, seed=5), shard(n, 1, 0, world, seed=5))
    assert list(shard(n, 0, 0, 1, shuffle=False)) == list(range(n))


def test_refusals_name_what_they_refuse(tmp_path):
    from xmm_superres_denoise.data.datamodule import make_splits, split_bases
    from xmm_superres_denoise.data.dataset import XmmDataset, inflate_files
    a = np.arange(20, dtype=np.int32).reshape(4, 5)
    good = dt.write_fits(str(tmp_path / "good.fits.gz"), a)
    bz = dt.write_fits(str(tmp_path / "bzero.fits.gz"), a, extra=[("BZERO", "32768")])
    with pytest.raises(ValueError, match="bzero.fits.gz.*BZERO"):
        inflate_files([good, bz], (4, 5))
    wrong = dt.write_fits(str(tmp_path / "wrong.fits.gz"), np.zeros((5, 4), np.int32))
    with pytest.raises(ValueError, match="wrong.fits.gz.*shape 5 x 4"):
        inflate_files([good, wrong], (4, 5))
    flt = dt.write_fits(str(tmp_path / "float.fits.gz"), a.astype(np.float32), bitpix=-32)
    with pytest.raises(ValueError, match="float.fits.gz.*BITPIX -32"):
        inflate_files([good, flt], (4, 5))
    out, bitpix = inflate_files([good], (4, 5))
    assert bitpix == 32 and np.array_equal(out[0].byteswap().view(np.int32), a.ravel())
    # an empty match names the split key; an empty split names the split
    os.makedirs(tmp_path / "empty" / "sim_dataset" / "img" / "20ks" / "1x")
    os.makedirs(tmp_path / "empty" / "sim_dataset" / "img" / "100ks" / "2x")
    with pytest.raises(ValueError, match='No base_names.*"_mult_"'):
        XmmDataset(_cfg(tmp_path / "empty", agn=0, lr_bkg=0))
    root = dt.make_sim_tree(str(tmp_path / "two"), n_base=2, n_agn=1, n_bkg=1, shape=(4, 5), hr_mult=2, hr_exp=100)
    d = XmmDataset(_cfg(root))
    s = make_splits(d, seed=0)
    assert len(s["train"]) == 2
    with pytest.raises(ValueError, match="split 'val' is empty"):
        split_bases(d, s["val"], "val")
    with pytest.raises(ValueError, match="split 'test'.*not in the dataset"):
        split_bases(d, ["nonexistent"], "test")
    with pytest.raises(ValueError, match="clamp_max"):
        XmmDataset(_cfg(root).model_copy(update={"lr": _cfg(root).lr.model_copy(update={"clamp_max": 0.0})}))


def test_fit_still_refuses_restormer_and_swinfir():
    from xmm_superres_denoise.train import fit
    with pytest.raises(NotImplementedError, match="restormer: training Restormer is not on the MI355X engine"):
        fit("restormer", dataset_dir="/nonexistent")
    with pytest.raises(NotImplementedError, match="swinfir: training SwinFIR is not on the MI355X engine"):
        fit("swinfir", dataset_dir="/nonexistent")
