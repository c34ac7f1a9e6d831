"""FITS dataset trees for the dataset tests and tools/dataset_feed_speed.py: gzip FITS writers, the reference layout
(<root>/<name>/{img,agn,bkg}/<exp>ks/<mult>x/), a seeded synthetic tree, and the tree recorded in dataset_sim.npz."""
import gzip
import os

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))


def fits_bytes(a: np.ndarray, bitpix: int = 32, extra=()) -> bytes:
    cards = [("SIMPLE", "T"), ("BITPIX", str(bitpix)), ("NAXIS", "2"), ("NAXIS1", str(a.shape[1])), ("NAXIS2", str(a.shape[0]))]
    cards += list(extra)
    hdr = b"".join(f"{k:<8}= {v:>20}".ljust(80).encode() for k, v in cards) + b"END".ljust(80)
    hdr += b" " * (-len(hdr) % 2880)
    dt = {32: ">i4", -32: ">f4", 8: "u1"}[bitpix]
    data = np.ascontiguousarray(a).astype(dt).tobytes()
    return hdr + data + b"\0" * (-len(data) % 2880)


def write_fits(path, a: np.ndarray, bitpix: int = 32, extra=()) -> str:
    os.makedirs(os.path.dirname(path), exist_ok=True)
    b = fits_bytes(a, bitpix, extra)
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(b)
    else:
        with open(path, "wb") as f:
            f.write(b)
    return str(path)


def sim_path(root, name, kind, exp, mult, fname):
    return os.path.join(root, name, kind, f"{exp}ks", f"{mult}x", fname)


def make_sim_tree(root, n_base=10, n_agn=2, n_bkg=2, lr_exps=(20,), hr_exp=50, hr_mult=1, shape=(411, 403), seed=0,
                  name="sim_dataset", realisations=1, lam=0.05):
    """seeded Poisson counts in the reference layout: n_base images and n_agn AGN at every LR exposure (1x) and at hr_exp
    (hr_mult x), n_bkg backgrounds at every LR exposure.  Returns the dataset directory (pass as dataset_dir)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    for kind, n in (("img", n_base), ("agn", n_agn)):
        for i in range(n):
            stem = f"{kind}{i:03d}_gal" if kind == "img" else f"agn_abs_{i}.0_src"
            for exp in lr_exps:
                for r in range(realisations):
                    write_fits(sim_path(root, name, kind, exp, 1, f"{stem}_mult_1_{exp}ks_p_{r}-{realisations}.fits.gz"),
                               rng.poisson(lam * exp / 20, (H, W)).astype(np.int32))
            write_fits(sim_path(root, name, kind, hr_exp, hr_mult, f"{stem}_mult_{hr_mult}_{hr_exp}ks_p_0-0.fits.gz"),
                       rng.poisson(lam * hr_exp / 20 / hr_mult ** 2, (H * hr_mult, W * hr_mult)).astype(np.int32))
    for exp in lr_exps:
        for k in range(n_bkg):
            write_fits(sim_path(root, name, "bkg", exp, 1, f"background_mult_1_{exp}ks_{k:05d}.fits.gz"),
                       rng.poisson(lam / 4, (H, W)).astype(np.int32))
    return str(root)


def golden_tree(root, z=None):
    """writes the FITS files recorded in dataset_sim.npz (gzip, BITPIX 32) into root; returns {relative path: path}"""
    if z is None:
        z = np.load(os.path.join(GOLDEN, "dataset_sim.npz"))
    out = {}
    for i, rel in enumerate(str(n) for n in z["file_paths"]):
        out[rel] = write_fits(os.path.join(root, rel), z[f"file_{i}"].astype(np.int32))
    return out


def unpack_mask(z, which):
    """the detector masks of example_data.npz (bit-packed) as uint8 [H, W]"""
    shp = tuple(int(v) for v in z[f"mask{which}_shape"])
    return np.unpackbits(z[f"mask{which}_bits"])[:shp[0] * shp[1]].reshape(shp)
