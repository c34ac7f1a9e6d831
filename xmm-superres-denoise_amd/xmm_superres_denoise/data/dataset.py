"""XmmDataset (reference data/dataset.py:77-270) with a device-resident sample pool.

Discovery and matching are the reference's (data/tools.py: find_img_dirs / find_img_files / match_file_list): LR images at
`<img_dir>/<exp>ks/**/1x` for every `lr.exps`, HR images at `<hr.exp>ks/**/<res_mult>x` (`<res_mult>x_comb` with comb_hr),
AGN images matched the same way under `agn_dir`, backgrounds under `bkg_dir` at the LR exposures; real data (`type = real`)
matches `<exp>ks/` files on `_image_split_` and has no AGN or background.  dataset_size = base names x len(lr.exps) x agn x bkg.

`build_pool` inflates every file the given base names can reach, once, with at most 16 host threads, into two device pools of
raw FITS words (LR slots of Hin x Win, HR slots).  The host only gunzips, parses the header and copies the data block.
`batch(indices, epoch)` then makes one `xsd_compose_batch` launch per resolution: sum, detector mask, upsample, pad and
normalize all run on the device, bitwise equal to the reference's `_load_and_combine_simulations` + `Normalize`.

Sample indices: sample s of a dataset with B base names and E LR exposures is base `s % B`, LR exposure `(s // B) % E`, replica
`s // (B E)` (one per agn x bkg combination).  With one exposure (the reference's default) that is the reference's
`load_sample` map (base = idx % base_name_count, exposure 0).  With several, the reference's map `(idx % E, idx % B)` cannot
reach every (base, exposure) pair, so this one enumerates them instead.

Random choices (which realisation of the LR / HR image, which AGN and its realisations, which background) come from a seeded
torch.Generator: one table of uniforms per (seed, epoch) over the whole dataset, row s for sample s.  A sample therefore depends
on neither the batch size, the rank count nor the order it is drawn in.  Python's `random` stream, which the reference draws
from (`sample`, `randint`, `DataFrame.sample`), is not reproduced.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from xmm_superres_denoise.config.config import DatasetCfg, DatasetType
from xmm_superres_denoise.data.tools import find_img_dirs, find_img_files, match_file_list, read_fits_block, read_fits_primary

MAX_HOST_THREADS = 16
_STRETCH = ("linear", "sqrt", "asinh", "log")


def inflate_files(paths: Sequence[Path], shape, out: Optional[np.ndarray] = None, threads: int = MAX_HOST_THREADS):
    """Gunzip + header-parse `paths` into `out` [len(paths), H*W] uint32 (raw FITS words), at most `threads` host threads.
    Returns (out, bitpix).  Refuses, naming the file: BITPIX other than 32 / -32, BZERO / BSCALE, a shape other than `shape`,
    and a BITPIX that differs from the first file's (one pool holds one word type)."""
    H, W = shape
    if out is None:
        out = np.empty((len(paths), H * W), dtype=np.uint32)
    kinds = [None] * len(paths)

    def one(i):
        bitpix, shp, words = read_fits_block(paths[i])
        if shp != (H, W):
            raise ValueError(f"{paths[i]}: shape {shp[0]} x {shp[1]}, expected {H} x {W}")
        out[i] = words
        kinds[i] = bitpix

    if paths:
        with ThreadPoolExecutor(max_workers=max(1, min(threads, MAX_HOST_THREADS, len(paths)))) as ex:
            list(ex.map(one, range(len(paths))))
        for p, k in zip(paths, kinds):
            if k != kinds[0]:
                raise ValueError(f"{p}: BITPIX {k}, but {paths[0]} has {kinds[0]} (a pool holds one word type)")
    return out, (kinds[0] if paths else 32)


class _Pool:
    """A device pool: `words` int32 [n_slots, H*W] of raw FITS words."""

    def __init__(self, files: List[Path], shape, device, max_pool_bytes: Optional[int], what: str):
        self.files, self.shape = files, tuple(shape)
        H, W = self.shape
        self.nbytes = len(files) * H * W * 4
        if device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(device)
            cap = free if max_pool_bytes is None else min(int(max_pool_bytes), free)
            if self.nbytes > cap:
                raise MemoryError(f"{what} pool: {len(files)} files x {H} x {W} words = {self.nbytes / 2**20:.1f} MiB does not fit: "
                                  f"max_pool_bytes {max_pool_bytes}, free device memory {free / 2**20:.1f} MiB")
        elif max_pool_bytes is not None and self.nbytes > max_pool_bytes:
            raise MemoryError(f"{what} pool: {self.nbytes / 2**20:.1f} MiB exceeds max_pool_bytes {max_pool_bytes}")
        self.words = torch.empty((len(files), H * W), dtype=torch.int32, device=device)
        chunk = max(1, (256 << 20) // max(1, H * W * 4))       # stage at most ~256 MiB of host memory at a time
        host = torch.empty((min(chunk, max(1, len(files))), H * W), dtype=torch.int32, pin_memory=device.type == "cuda")
        self.bitpix = None
        for c0 in range(0, len(files), chunk):
            part = files[c0:c0 + chunk]
            _, bp = inflate_files(part, self.shape, host.numpy().view(np.uint32)[:len(part)])
            if self.bitpix is not None and bp != self.bitpix:
                raise ValueError(f"{part[0]}: BITPIX {bp}, but {files[0]} has {self.bitpix} (a pool holds one word type)")
            self.bitpix = bp
            self.words[c0:c0 + len(part)].copy_(host[:len(part)])
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()     # the staging buffer is reused / freed after this


class XmmDataset:
    """reference XmmDataset(config, comb_hr_img, transform, normalize); `normalize` = apply Normalize(lr.clamp_max, hr.clamp_max,
    scaling) as `__getitem__` does (data/datamodule.py:31-35 always passes it).  `transform` is None in the reference's
    datamodule (:22-29) and is not taken here."""

    def __init__(self, config: DatasetCfg, comb_hr_img: bool = False, normalize: bool = True, seed: int = 0):
        self.config, self.seed, self.normalize = config, int(seed), bool(normalize)
        real = config.type is DatasetType.REAL
        if config.type not in (DatasetType.SIM, DatasetType.REAL):
            raise ValueError(f"Dataset type {config.type} not known, options: 'real', 'sim'")
        split_key = "_mult_" if not real else "_image_split_"
        self.split_key = split_key
        lr_mult = "1x" if not real else ""
        if real and config.hr is not None and config.hr.exp:
            hr_mult = ""
        elif not real and comb_hr_img:
            hr_mult = f"{config.res_mult}x_comb"
        else:
            hr_mult = f"{config.res_mult}x"
        self.exps = list(config.lr.exps)
        lr_files = find_img_files(find_img_dirs(config.img_dir, self.exps, lr_mult))
        hr_files = None
        if not (real and config.hr is None):
            hr_files = find_img_files(find_img_dirs(config.img_dir, [config.hr.exp], hr_mult))
        self.lr_img_files, self.hr_img_files, self.base_name_count = match_file_list(lr_files, hr_files, split_key)
        self.base_names = list(self.lr_img_files.index)
        # real data: ImageUpsample(res_mult) on the HR image when the resolutions differ (:128-133); res_mult is 1 for real
        # data, so as written that upsample is the identity -- kept as written
        self.hr_upsample = config.res_mult if (real and config.hr is not None and config.hr.res != config.lr.res) else 1
        self.dataset_size = self.base_name_count * len(self.exps)
        self.n_agn = self.n_bkg = 1
        self.lr_agn_files = self.hr_agn_files = None
        self.base_agn_count = 0
        if config.agn > 0 and not real:
            self.n_agn = int(config.agn)
            self.dataset_size *= self.n_agn
            la = find_img_files(find_img_dirs(config.agn_dir, self.exps, lr_mult))
            ha = find_img_files(find_img_dirs(config.agn_dir, [config.hr.exp], hr_mult))
            self.lr_agn_files, self.hr_agn_files, self.base_agn_count = match_file_list(la, ha, split_key)
        self.lr_bkg_files = None
        if config.lr.bkg > 0 and not real:
            self.n_bkg = int(config.lr.bkg)
            self.dataset_size *= self.n_bkg
            bf = find_img_files(find_img_dirs(config.bkg_dir, self.exps, lr_mult))
            amt = min(len(v) for v in bf.values())
            if amt == 0:
                raise ValueError(f"no background files under {config.bkg_dir} for one of the exposures {self.exps}")
            # the reference keeps a random subset of `amt` files per exposure (:193-197); here a seeded one, in file order
            g = torch.Generator().manual_seed(self.seed)
            self.lr_bkg_files = {exp: [files[i] for i in sorted(torch.randperm(len(files), generator=g)[:amt].tolist())]
                                 for exp, files in bf.items()}
        self.lr_res, self.hr_res = config.lr.res, (config.hr.res if config.hr is not None else None)
        for what, v in (("lr", config.lr.clamp_max), ("hr", config.hr.clamp_max if config.hr is not None else 1.0)):
            if self.normalize and not v > 0:
                raise ValueError(f"{what}.clamp_max = {v}: normalising by each image's own maximum (normalize.py:72-74) is a "
                                 "per-sample reduction the batched compose does not do; set clamp_max > 0")
        self.lr_pool = self.hr_pool = None
        self._tables = {}

    def __len__(self):
        return self.dataset_size

    # ---- index map ---------------------------------------------------------------------------------------------------------
    def decode(self, indices):
        """sample index -> (base, lr exposure index, replica); see the module docstring"""
        s = np.asarray(indices, dtype=np.int64)
        if s.size and (s.min() < 0 or s.max() >= self.dataset_size):
            bad = int(s[(s < 0) | (s >= self.dataset_size)][0])
            raise IndexError(f"sample index {bad} outside the dataset's {self.dataset_size} samples")
        nb, ne = self.base_name_count, len(self.exps)
        return s % nb, (s // nb) % ne, s // (nb * ne)

    def samples_of(self, base_indices) -> np.ndarray:
        """every sample of the given base names: each (lr exposure, agn, bkg) combination, base-major in the given order"""
        b = np.asarray(list(base_indices), dtype=np.int64)
        nb, ne, nr = self.base_name_count, len(self.exps), self.n_agn * self.n_bkg
        rest = np.arange(ne * nr, dtype=np.int64)           # e + ne * rep
        return (b[:, None] + nb * rest[None, :]).reshape(-1)

    # ---- pool ----------------------------------------------------------------------------------------------------------------
    def build_pool(self, base_indices=None, device=None, max_pool_bytes: Optional[int] = None) -> "XmmDataset":
        """Inflate every file the given base names (default: all) can reach -- their LR / HR images, every AGN image, every kept
        background -- into the device pools, and read the detector masks once as uint8 device tensors."""
        device = torch.device(device if device is not None else "cuda")
        cfg = self.config
        bases = sorted(set(range(self.base_name_count) if base_indices is None else (int(b) for b in base_indices)))
        nb, ne = self.base_name_count, len(self.exps)
        lr_files, hr_files = [], []
        # slot tables: [offset, count] per (base, exp) / base / (agn, exp) / agn; offset -1 = not pooled
        self._lr_img = np.full((nb, ne, 2), -1, dtype=np.int64)
        self._hr_img = np.full((nb, 2), -1, dtype=np.int64)

        def put(lst, files):
            off = len(lst)
            lst.extend(files)
            return off, len(files)

        for b in bases:
            for e in range(ne):
                self._lr_img[b, e] = put(lr_files, self.lr_img_files.cell(b, e))
            if self.hr_img_files is not None:
                self._hr_img[b] = put(hr_files, self.hr_img_files.cell(b, 0))
        if self.lr_agn_files is not None:
            na = self.base_agn_count
            self._lr_agn = np.zeros((na, ne, 2), dtype=np.int64)
            self._hr_agn = np.zeros((na, 2), dtype=np.int64)
            for a in range(na):
                for e in range(ne):
                    self._lr_agn[a, e] = put(lr_files, self.lr_agn_files.cell(a, e))
                self._hr_agn[a] = put(hr_files, self.hr_agn_files.cell(a, 0))
        if self.lr_bkg_files is not None:
            self._bkg = np.zeros((ne, 2), dtype=np.int64)
            for e, exp in enumerate(self.exps):
                self._bkg[e] = put(lr_files, self.lr_bkg_files[exp])
        lr_shape = read_fits_block(lr_files[0])[1]
        self.lr_pool = _Pool(lr_files, lr_shape, device, max_pool_bytes, "LR")
        left = None if max_pool_bytes is None else max_pool_bytes - self.lr_pool.nbytes
        self.hr_pool = _Pool(hr_files, read_fits_block(hr_files[0])[1], device, left, "HR") if hr_files else None
        self.lr_mask = self._mask(cfg.lr.det_mask, self.lr_pool.shape, device)
        self.hr_mask = self._mask(cfg.hr.det_mask, self.hr_pool.shape, device) if self.hr_pool is not None else None
        self.device = device
        return self

    @staticmethod
    def _mask(path, shape, device):
        if path is None or str(path) == "":
            return None
        path = Path(path)
        if not path.is_file():
            raise FileNotFoundError(f"Detector mask does not exist at '{path}'!")
        m = read_fits_primary(path)
        if m.shape != tuple(shape):
            raise ValueError(f"{path}: detector mask of {m.shape[0]} x {m.shape[1]}, the images are {shape[0]} x {shape[1]}")
        if m.dtype != np.uint8:
            if not np.all((m >= 0) & (m <= 255) & (m == np.round(m))):
                raise ValueError(f"{path}: the detector mask must hold integers 0..255 (BITPIX 8)")
            m = m.astype(np.uint8)
        return torch.from_numpy(np.ascontiguousarray(m)).to(device)

    @property
    def pool_bytes(self) -> int:
        return (self.lr_pool.nbytes if self.lr_pool else 0) + (self.hr_pool.nbytes if self.hr_pool else 0)

    # ---- batches ---------------------------------------------------------------------------------------------------------------
    def _uniforms(self, epoch: int) -> np.ndarray:
        key = int(epoch)
        if key not in self._tables:
            g = torch.Generator().manual_seed(self.seed * 1_000_003 + key)
            self._tables = {key: torch.rand((self.dataset_size, 6), generator=g, dtype=torch.float64).numpy()}
        return self._tables[key]

    def slots(self, indices, epoch: int = 0):
        """host slot numbers of a batch: (lr img, lr agn | None, lr bkg | None, hr img | None, hr agn | None), int32 [B] each"""
        if self.lr_pool is None:
            raise RuntimeError("build_pool() first")
        s = np.asarray(indices, dtype=np.int64).reshape(-1)
        b, e, _ = self.decode(s)
        u = self._uniforms(epoch)[s]

        def pick(tab, col):
            return tab[..., 0] + np.minimum((u[:, col] * tab[..., 1]).astype(np.int64), tab[..., 1] - 1)

        lr_t = self._lr_img[b, e]
        if (lr_t[:, 0] < 0).any():
            i = int(np.nonzero(lr_t[:, 0] < 0)[0][0])
            raise IndexError(f"sample {int(s[i])} (base name {self.base_names[b[i]]}) is not in this dataset's pool: "
                             "build_pool() was given other base names")
        lr_img = pick(lr_t, 0)
        hr_img = pick(self._hr_img[b], 1) if self.hr_pool is not None else None
        lr_agn = hr_agn = lr_bkg = None
        if self.lr_agn_files is not None:
            a = np.minimum((u[:, 2] * self.base_agn_count).astype(np.int64), self.base_agn_count - 1)
            lr_agn = pick(self._lr_agn[a, e], 3)
            hr_agn = pick(self._hr_agn[a], 4) if self.hr_pool is not None else None
        if self.lr_bkg_files is not None:
            lr_bkg = pick(self._bkg[e], 5)
        cast = (lambda x: None if x is None else x.astype(np.int32))
        return cast(lr_img), cast(lr_agn), cast(lr_bkg), cast(hr_img), cast(hr_agn)

    def batch(self, indices, epoch: int = 0):
        """-> (lr [B,1,lr.res,lr.res], hr [B,1,hr.res,hr.res] or None) on the pool's device: one xsd_compose_batch launch per
        resolution; the slot numbers travel in its argument block."""
        from xmm_superres_denoise.engine import compose_batch
        cfg = self.config
        lr_img, lr_agn, lr_bkg, hr_img, hr_agn = self.slots(indices, epoch)
        stretch = cfg.scaling
        H, W = self.lr_pool.shape
        lr = compose_batch(self.lr_pool.words, lr_img, lr_agn, lr_bkg, self.lr_mask, H, W, self.lr_res,
                           cfg.lr.clamp_max if self.normalize else None, stretch, 1, self.lr_pool.bitpix == 32, True)
        hr = None
        if self.hr_pool is not None:
            H, W = self.hr_pool.shape
            hr = compose_batch(self.hr_pool.words, hr_img, hr_agn, None, self.hr_mask, H, W, self.hr_res,
                               cfg.hr.clamp_max if self.normalize else None, stretch, self.hr_upsample, self.hr_pool.bitpix == 32, True)
        return lr, hr

    def file_names(self, indices, epoch: int = 0):
        """the files each sample of a batch is composed of (lr img, lr agn, lr bkg, hr img, hr agn; None = absent)"""
        sl = self.slots(indices, epoch)
        pools = (self.lr_pool, self.lr_pool, self.lr_pool, self.hr_pool, self.hr_pool)
        return [tuple(None if x is None else pools[k].files[int(x[i])].name for k, x in enumerate(sl)) for i in range(len(sl[0]))]
