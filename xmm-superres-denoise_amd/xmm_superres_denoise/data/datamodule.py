"""Splits and rank shards of an XmmDataset (reference data/datamodule.py:66-190), without Lightning or DataLoader workers.

Splits: simulations 0.8 / 0.1 / 0.1 over the base names, real data 0.7 / 0.15 / 0.15 over the LR files of the first LR
exposure (one per base name), with torch's `random_split` under a fixed-seed torch.Generator.  The first run writes them as a
JSON of base names (sim) / LR file names (real); later runs read that file back.  The reference's split is unseeded and stored
as pickled index arrays; those files are not read here (unpickling executes code).

A split's samples are every (base name, LR exposure, agn, bkg) combination of its base names (XmmDataset.samples_of).  With
one exposure and agn, bkg <= 1 -- the reference's default -- that is the reference's index list itself.  The reference's
`_load_indices` multiplies the indices by (i + 1) otherwise, which yields out-of-range or repeated indices; it is not
reproduced.

Rank shards follow torch's DistributedSampler: a permutation from seed + epoch (train only), padded by wrap-around to a
multiple of the world size, rank r takes [r::world].  Every rank pools all of its split's files (`XmmDataModule.setup`),
since over the epochs a rank's shard reaches any of them.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch
from torch.utils.data import DistributedSampler, random_split

from xmm_superres_denoise.config.config import DatasetCfg, DatasetType
from xmm_superres_denoise.data.dataset import XmmDataset

SPLITS = ("train", "val", "test")


def split_fractions(cfg: DatasetCfg):
    return [0.8, 0.1, 0.1] if cfg.type is DatasetType.SIM else [0.7, 0.15, 0.15]


def make_splits(dataset: XmmDataset, seed: int = 0) -> Dict[str, List[str]]:
    """{"train" | "val" | "test": names}: base names (sim) or LR file names of the first LR exposure (real)"""
    g = torch.Generator().manual_seed(int(seed))
    parts = random_split(range(dataset.base_name_count), split_fractions(dataset.config), generator=g)
    return {name: [_split_name(dataset, i) for i in p.indices] for name, p in zip(SPLITS, parts)}


def _split_name(dataset: XmmDataset, base: int) -> str:
    if dataset.config.type is DatasetType.SIM:
        return dataset.base_names[base]
    return dataset.lr_img_files.cell(base, 0)[0].name


def load_or_make_splits(dataset: XmmDataset, path: str, seed: int = 0) -> Dict[str, List[str]]:
    """reads the split JSON at `path`, or makes it (seeded) and writes it there first"""
    if os.path.exists(path):
        with open(path) as f:
            d = json.load(f)
        missing = [s for s in SPLITS if s not in d]
        if missing:
            raise ValueError(f"{path}: split file without {missing}")
        return {s: list(d[s]) for s in SPLITS}
    d = make_splits(dataset, seed)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"type": str(dataset.config.type), "seed": int(seed), **d}, f, indent=1)
    return d


def split_bases(dataset: XmmDataset, names: List[str], split: str) -> List[int]:
    """names of a split -> base indices in this dataset; refuses names the dataset does not have, and an empty split"""
    if dataset.config.type is DatasetType.SIM:
        lookup = {b: i for i, b in enumerate(dataset.base_names)}
    else:
        lookup = {}
        for i in range(dataset.base_name_count):
            for p in dataset.lr_img_files.cell(i, 0):
                lookup[p.name] = i
    unknown = [n for n in names if n not in lookup]
    if unknown:
        raise ValueError(f"split '{split}': {len(unknown)} name(s) not in the dataset, e.g. {unknown[0]}")
    if not names:
        raise ValueError(f"split '{split}' is empty: {dataset.base_name_count} base name(s) split "
                         f"{' / '.join(str(f) for f in split_fractions(dataset.config))} leave nothing for it")
    return [lookup[n] for n in names]


def shard(n: int, epoch: int, rank: int = 0, world: int = 1, shuffle: bool = True, seed: int = 0) -> np.ndarray:
    """positions 0..n-1 of a split that `rank` visits in `epoch` (torch DistributedSampler, drop_last = False)"""
    s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed, drop_last=False)
    s.set_epoch(epoch)
    return np.asarray(list(s), dtype=np.int64)


class XmmDataModule:
    """reference XmmDataModule(config): `prepare_data` makes / reads the split JSON, `setup(stage)` selects the splits' samples and
    builds the device pools over the base names those splits reach."""

    def __init__(self, config: DatasetCfg, splits_path: str, seed: int = 0, rank: int = 0, world: int = 1):
        if config.type is DatasetType.BORING:
            raise ValueError("type = boring: use train.fit without a dataset (random tiles)")
        self.config, self.splits_path, self.seed, self.rank, self.world = config, splits_path, int(seed), rank, world
        self.dataset = XmmDataset(config, comb_hr_img=config.comb_hr, seed=seed)
        self.samples: Dict[str, np.ndarray] = {}

    def prepare_data(self):
        self.split_names = load_or_make_splits(self.dataset, self.splits_path, self.seed)
        return self.split_names

    def setup(self, stage: str = "fit", device=None, max_pool_bytes: Optional[int] = None):
        if not hasattr(self, "split_names"):
            self.prepare_data()
        names = ("train", "val", "test") if stage == "fit" else ("test",)
        bases = {}
        for s in names:
            bases[s] = split_bases(self.dataset, self.split_names[s], s)
            self.samples[s] = self.dataset.samples_of(bases[s])
        self.dataset.build_pool(sorted({b for v in bases.values() for b in v}), device=device, max_pool_bytes=max_pool_bytes)
        return self

    def batches(self, split: str, batch_size: int, epoch: int = 0):
        """this rank's batches of a split, as sample-index arrays (train: shuffled per epoch)"""
        sm = self.samples[split]
        pos = shard(len(sm), epoch, self.rank, self.world, shuffle=split == "train", seed=self.seed)
        idx = sm[pos]
        return [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]

    def num_batches(self, split: str, batch_size: int) -> int:
        return math.ceil(math.ceil(len(self.samples[split]) / self.world) / batch_size)
