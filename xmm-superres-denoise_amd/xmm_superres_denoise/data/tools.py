"""Host-side pieces of the input path the engine needs around its kernels (reference data/tools.py:79-126,
data/dataset.py:24-49): a dependency-free FITS primary-HDU reader (the reference uses astropy) and the fused
detector-mask * pad (* normalize) entry point."""
from __future__ import annotations

import gzip
from pathlib import Path
from typing import Dict, List, Optional, Set, Tuple

import numpy as np
import torch

from xmm_superres_denoise.engine import mask_pad_normalize as _hip_mask_pad_normalize


def load_fits(fits_path) -> torch.Tensor:
    """PRIMARY HDU image as float32 [1,H,W] (reference data/tools.py:79-86)."""
    a = read_fits_primary(fits_path)
    return torch.from_numpy(a.astype(np.float32)).unsqueeze(0)


def read_fits_primary(path) -> np.ndarray:
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        raw = f.read()
    hdr, off, done = {}, 0, False
    while not done:
        blk = raw[off:off + 2880]
        if len(blk) < 2880:
            raise ValueError(f"{path}: truncated FITS header")
        off += 2880
        for i in range(36):
            card = blk[i * 80:(i + 1) * 80].decode("ascii", "replace")
            key = card[:8].strip()
            if key == "END":
                done = True
                break
            if card[8:10] == "= ":
                hdr[key] = card[10:].split("/")[0].strip().strip("'").strip()
    dt = {8: "u1", 16: ">i2", 32: ">i4", -32: ">f4", -64: ">f8"}[int(hdr["BITPIX"])]
    n1, n2 = int(hdr["NAXIS1"]), int(hdr["NAXIS2"])
    a = np.frombuffer(raw, dtype=dt, count=n1 * n2, offset=off).reshape(n2, n1)
    bz, bs = float(hdr.get("BZERO", 0.0)), float(hdr.get("BSCALE", 1.0))
    if bz != 0.0 or bs != 1.0:
        a = a.astype(np.float64) * bs + bz
    return np.ascontiguousarray(a.astype(a.dtype.newbyteorder("=")))


def reshape_img_to_res(res: int, img: torch.Tensor) -> torch.Tensor:
    """Centred zero pad / crop of [1,H,W] (or [B,H,W]) to [*,res,res] on the GPU (reference data/tools.py:103-126)."""
    return _hip_mask_pad_normalize(img.contiguous(), None, res, None)[:, 0]


def load_and_prepare(counts: torch.Tensor, det_mask: torch.Tensor | None, res: int, max_val: float | None = None,
                     stretch: str = "linear") -> torch.Tensor:
    """counts [B,Hin,Win] (int32 or float32, CUDA) -> img *= mask -> pad to res -> optional normalize, one kernel
    (reference data/dataset.py:41-47 + :267-268)."""
    return _hip_mask_pad_normalize(counts.contiguous(), det_mask, res, max_val, stretch)


# ---- file discovery and matching (reference data/tools.py:24-45,129-201), host only ------------------------------------------
def find_img_dirs(parent: Path, exps, res_mult_dir: str) -> Dict[int, List[Path]]:
    """`<exp>ks/**/<res_mult_dir>` (or `<exp>ks/` when res_mult_dir is empty) under parent, per exposure.  The directories are
    sorted (the reference keeps the filesystem's glob order; they agree whenever an exposure has one such directory)."""
    if isinstance(exps, int):
        exps = [exps]
    res: Dict[int, List[Path]] = {}
    for exp in exps:
        pattern = f"{exp}ks/**/{res_mult_dir}" if res_mult_dir else f"{exp}ks/"
        dirs = sorted(Path(parent).glob(pattern))
        if not dirs:
            raise FileNotFoundError(f"no directory matches {Path(parent) / pattern}")
        res[exp] = dirs
    return res


def find_img_files(exp_dirs_dict: Dict[int, List[Path]]) -> Dict[int, List[Path]]:
    return {exp: [f for d in dirs for f in get_fits_files(d)] for exp, dirs in exp_dirs_dict.items()}


def get_fits_files(dataset_dir: Path) -> List[Path]:
    dataset_dir = Path(dataset_dir)
    if not dataset_dir.is_dir():
        raise FileNotFoundError(f"Dataset directory {dataset_dir} does not exist!")
    return sorted(list(dataset_dir.glob("*.fits")) + list(dataset_dir.glob("*.fits.gz")))


def get_base_names(img_dict, split_key: str) -> Set[str]:
    if isinstance(img_dict, dict):
        # an exposure without a file of some base name drops that base name
        return set.intersection(*[{f.name.split(split_key)[0] for f in files} for files in img_dict.values()])
    return {f.name.split(split_key)[0] for f in img_dict}


def filter_img_dict(img_dict: Dict[int, List[Path]], base_names: set, split_key: str) -> Dict[int, Dict[str, List[Path]]]:
    out = {exp: {b: [] for b in base_names} for exp in img_dict}
    for exp, files in img_dict.items():
        for f in files:
            b = f.name.split(split_key)[0]
            if b in base_names:
                out[exp][b].append(f)
    return out


class FileTable:
    """What the reference's `pd.DataFrame.from_dict(filter_img_dict(...)).sort_index()` holds: rows = base names (sorted),
    columns = exposures (in the given order), cell = the list of that base name's files (its realisations)."""

    def __init__(self, d: Dict[int, Dict[str, List[Path]]]):
        self.columns = list(d)
        self.index = sorted(next(iter(d.values()))) if d else []
        self.cells = [[list(d[exp][b]) for exp in self.columns] for b in self.index]

    def cell(self, row: int, col: int) -> List[Path]:
        return self.cells[row][col]

    def column(self, exp: int) -> List[List[Path]]:
        c = self.columns.index(exp)
        return [r[c] for r in self.cells]

    def names(self) -> List[List[List[str]]]:
        return [[[p.name for p in cell] for cell in row] for row in self.cells]

    def __len__(self):
        return len(self.index)


def match_file_list(lr_dict: Dict[int, List[Path]], hr_dict: Optional[Dict[int, List[Path]]], split_key: str
                    ) -> Tuple[FileTable, Optional[FileTable], int]:
    lr_base = get_base_names(lr_dict, split_key)
    hr_base = get_base_names(hr_dict, split_key) if hr_dict is not None else lr_base
    base_names = lr_base & hr_base
    if not base_names:
        raise ValueError(f'No base_names could be found in both given dictionaries with split_key "{split_key}"!')
    lr = FileTable(filter_img_dict(lr_dict, base_names, split_key))
    hr = FileTable(filter_img_dict(hr_dict, base_names, split_key)) if hr_dict is not None else None
    return lr, hr, len(base_names)


def read_fits_block(path) -> Tuple[int, Tuple[int, int], np.ndarray]:
    """(BITPIX, (NAXIS2, NAXIS1), data block as raw uint32 words in FITS byte order) of the primary HDU.  No conversion: the
    device does the byte swap and the int -> float.  Refuses what the device path cannot take, naming the file."""
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        raw = f.read()
    hdr, off = _parse_header(raw, path)
    bitpix = int(hdr["BITPIX"])
    if bitpix not in (32, -32):
        raise ValueError(f"{path}: BITPIX {bitpix} (the sample pool takes 32 or -32)")
    bz, bs = float(hdr.get("BZERO", 0.0)), float(hdr.get("BSCALE", 1.0))
    if bz != 0.0 or bs != 1.0:
        raise ValueError(f"{path}: BZERO = {bz:g}, BSCALE = {bs:g} (the sample pool takes raw words only: BZERO 0, BSCALE 1)")
    n1, n2 = int(hdr["NAXIS1"]), int(hdr["NAXIS2"])
    if len(raw) < off + 4 * n1 * n2:
        raise ValueError(f"{path}: truncated data block")
    return bitpix, (n2, n1), np.frombuffer(raw, dtype=np.uint32, count=n1 * n2, offset=off)


def _parse_header(raw: bytes, path):
    hdr, off = {}, 0
    while True:
        blk = raw[off:off + 2880]
        if len(blk) < 2880:
            raise ValueError(f"{path}: truncated FITS header")
        off += 2880
        for i in range(36):
            card = blk[i * 80:(i + 1) * 80].decode("ascii", "replace")
            key = card[:8].strip()
            if key == "END":
                return hdr, off
            if card[8:10] == "= ":
                hdr[key] = card[10:].split("/")[0].strip().strip("'").strip()
