"""Writes tests/golden/dataset_sim.npz from the reference's own data/tools.py and data/dataset.py (imported by path; astropy,
loguru, tqdm and enum.StrEnum stubbed as SURVEY.md section 8c describes).  Needs the reference checkout (argument 1, default
../reference/xmm_superres_denoise next to this repository); the tests only read the npz.

It links a subset of the reference's data/example_data/sim -- 2 base names, 2 AGN, 2 backgrounds at 20 ks and 50 ks (1x) and
100 ks (2x) -- into the reference layout <tmp>/sim_dataset/{img,agn,bkg}/<exp>ks/<mult>x/, and records:
  * every file's counts (uint16; the files are BITPIX 32) and its path in the tree (file_paths / file_<i>);
  * the reference's base_name_count, dataset_size and matched file lists for lr.exps [20] and [20, 50] (HR: 100 ks 2x);
  * the reference's real-type matching (_image_split_, 20 -> 50 ks) on placeholders named like the 9 example obsids' files;
  * for 4 explicit (img, agn, bkg, hr img, hr agn) combinations -- two DN (HR 50 ks 1x, hr.res 416), two SR (HR 100 ks 2x,
    hr.res 832), the second of each with the detector masks -- the SHA-256 and float64 sum of the reference's float32 LR and
    HR tensors after _load_and_combine_simulations + Normalize(lr_max, hr_max, "sqrt").normalize_lr_image / _hr_image."""
import enum
import glob
import hashlib
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LR_MAX, HR_MAX = 0.0022336, 0.0005584


def _stub_modules(fits_reader):
    if not hasattr(enum, "StrEnum"):
        class StrEnum(str, enum.Enum):
            def __str__(self):
                return self.value
        enum.StrEnum = StrEnum
    astropy = types.ModuleType("astropy")
    io = types.ModuleType("astropy.io")
    fits = types.ModuleType("astropy.io.fits")
    fits.getdata = lambda path, ext="PRIMARY": fits_reader(path)
    astropy.io, io.fits = io, fits
    loguru = types.ModuleType("loguru")
    loguru.logger = types.SimpleNamespace(**{k: (lambda *a, **kw: None) for k in ("info", "success", "warning", "debug", "error")})
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, *a, **kw: it
    sys.modules.update({"astropy": astropy, "astropy.io": io, "astropy.io.fits": fits, "loguru": loguru, "tqdm": tqdm})


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def _fits_reader(path):
    """astropy's getdata for these files: the primary HDU in its FITS (big-endian) dtype"""
    import gzip
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        raw = f.read()
    hdr, off = {}, 0
    while True:
        blk = raw[off:off + 2880]
        off += 2880
        cards = [blk[i * 80:(i + 1) * 80].decode() for i in range(36)]
        if any(c[:8].strip() == "END" for c in cards):
            for c in cards:
                if c[8:10] == "= ":
                    hdr[c[:8].strip()] = c[10:].split("/")[0].strip()
            break
        for c in cards:
            if c[8:10] == "= ":
                hdr[c[:8].strip()] = c[10:].split("/")[0].strip()
    dt = {8: "u1", 32: ">i4", -32: ">f4"}[int(hdr["BITPIX"])]
    n1, n2 = int(hdr["NAXIS1"]), int(hdr["NAXIS2"])
    assert float(hdr.get("BZERO", 0)) == 0 and float(hdr.get("BSCALE", 1)) == 1
    return np.frombuffer(raw, dtype=dt, count=n1 * n2, offset=off).reshape(n2, n1)


def main(ref):
    _stub_modules(_fits_reader)
    sys.path.insert(0, ref)
    for pkg in ("data", "transforms", "config"):          # bare packages: their __init__ pulls in lightning
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(ref, pkg)]
        sys.modules[pkg] = m
    _load("config.config", os.path.join(ref, "config", "config.py"))
    norm_mod = _load("transforms.normalize", os.path.join(ref, "transforms", "normalize.py"))
    up_mod = _load("transforms.imageupsample", os.path.join(ref, "transforms", "imageupsample.py"))
    sys.modules["transforms"].Normalize, sys.modules["transforms"].ImageUpsample = norm_mod.Normalize, up_mod.ImageUpsample
    tools = _load("data.tools", os.path.join(ref, "data", "tools.py"))
    ds = _load("data.dataset", os.path.join(ref, "data", "dataset.py"))
    from config.config import DatasetCfg

    ex = os.path.join(os.path.dirname(ref), "data", "example_data", "sim")
    imgs = sorted(os.path.basename(p).split("_mult_")[0] for p in glob.glob(os.path.join(ex, "20ks", "img", "1x", "*")))[:2]
    agns = sorted(os.path.basename(p).split("_mult_")[0] for p in glob.glob(os.path.join(ex, "20ks", "agn", "1x", "*")))[:2]
    tmp = tempfile.mkdtemp()
    rels = []
    try:
        for kind, src_kind, bases in (("img", "img", imgs), ("agn", "agn", agns)):
            for exp, mult in ((20, 1), (50, 1), (100, 2)):
                for p in sorted(glob.glob(os.path.join(ex, f"{exp}ks", src_kind, f"{mult}x", "*"))):
                    if os.path.basename(p).split("_mult_")[0] in bases:
                        rels.append((os.path.join("sim_dataset", kind, f"{exp}ks", f"{mult}x", os.path.basename(p)), p))
        for exp in (20, 50):
            for p in sorted(glob.glob(os.path.join(ex, f"{exp}ks", "background", "1x", "*")))[:2]:
                rels.append((os.path.join("sim_dataset", "bkg", f"{exp}ks", "1x", os.path.basename(p)), p))
        for rel, p in rels:
            os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
            os.symlink(p, os.path.join(tmp, rel))
        out = {"file_paths": np.array([r for r, _ in rels])}
        for i, (_, p) in enumerate(rels):
            a = _fits_reader(p)
            assert a.dtype == np.dtype(">i4") and 0 <= a.min() and a.max() < 65536
            out[f"file_{i}"] = a.astype(np.uint16)         # counts < 65536: stored as uint16, written back as BITPIX 32

        def cfg(exps, hr_exp, hr_res, lr_mask="", hr_mask=""):
            return DatasetCfg(agn=1, batch_size=1, check_files=False, debug=True, comb_hr=False, crop_mode="center", directory=tmp,
                              mode="img", name="sim_dataset", scaling="sqrt", type="sim",
                              lr=dict(bkg=1, det_mask=lr_mask, exps=exps, clamp_max=LR_MAX, res=416),
                              hr=dict(det_mask=hr_mask, agn=True, exp=hr_exp, clamp_max=HR_MAX, res=hr_res))

        for tag, exps in (("e20", [20]), ("e20_50", [20, 50])):
            d = ds.XmmDataset(cfg(exps, 100, 832), comb_hr_img=False)
            out[f"{tag}_base_name_count"] = np.array([d.base_name_count])
            out[f"{tag}_dataset_size"] = np.array([d.dataset_size])
            out[f"{tag}_base_names"] = np.array(list(d.lr_img_files.index))
            out[f"{tag}_lr_files"] = np.array([[";".join(p.name for p in d.lr_img_files.iloc[b].iloc[e]) for e in range(len(exps))]
                                                for b in range(d.base_name_count)])
            out[f"{tag}_hr_files"] = np.array([";".join(p.name for p in d.hr_img_files.iloc[b].iloc[0]) for b in range(d.base_name_count)])
            out[f"{tag}_agn_count"] = np.array([d.base_agn_count])
        # real-type matching on placeholders named like the example obsids' files
        real = os.path.join(os.path.dirname(ref), "data", "example_data", "real")
        names = {e: sorted(os.path.basename(p) for p in glob.glob(os.path.join(real, f"{e}ks", "*.fits"))) for e in (20, 50)}
        rt = os.path.join(tmp, "real")
        for e, ns in names.items():
            os.makedirs(os.path.join(rt, f"{e}ks"))
            for n in ns:
                open(os.path.join(rt, f"{e}ks", n), "w").close()
        lr_d = tools.find_img_files(tools.find_img_dirs(__import__("pathlib").Path(rt), [20], ""))
        hr_d = tools.find_img_files(tools.find_img_dirs(__import__("pathlib").Path(rt), [50], ""))
        lr_df, hr_df, n = tools.match_file_list(lr_d, hr_d, "_image_split_")
        out["real_names_20"], out["real_names_50"] = np.array(names[20]), np.array(names[50])
        out["real_base_names"] = np.array(list(lr_df.index))
        out["real_lr_files"] = np.array([";".join(p.name for p in lr_df.iloc[b].iloc[0]) for b in range(n)])
        out["real_hr_files"] = np.array([";".join(p.name for p in hr_df.iloc[b].iloc[0]) for b in range(n)])

        # 4 explicit combinations through the reference's _load_and_combine_simulations + Normalize("sqrt")
        z = np.load(os.path.join(HERE, "example_data.npz"))
        sys.path.insert(0, HERE)
        from dataset_tree import unpack_mask, write_fits
        masks = {}
        for w in ("1x", "2x"):
            masks[w] = write_fits(os.path.join(tmp, "masks", f"mask_{w}.fits"), unpack_mask(z, w), bitpix=8)
        P = lambda kind, exp, mult, base: [os.path.join(tmp, r) for r, _ in rels
                                           if r.startswith(os.path.join("sim_dataset", kind, f"{exp}ks", f"{mult}x"))
                                           and os.path.basename(r).startswith(base + "_mult_")][0]
        bkg20 = sorted(os.path.join(tmp, r) for r, _ in rels if "/bkg/20ks/" in r)
        normalize = norm_mod.Normalize(lr_max=LR_MAX, hr_max=HR_MAX, stretch_mode="sqrt")
        combos = [("dn", imgs[0], agns[1], 0, 50, 1, 416, False), ("dn", imgs[1], agns[0], 1, 50, 1, 416, True),
                  ("sr", imgs[1], agns[1], 1, 100, 2, 832, False), ("sr", imgs[0], agns[0], 0, 100, 2, 832, True)]
        rows = []
        for i, (kind, img, agn, k, hexp, hm, hres, masked) in enumerate(combos):
            lr_paths = (P("img", 20, 1, img), P("agn", 20, 1, agn), bkg20[k])
            hr_paths = (P("img", hexp, hm, img), P("agn", hexp, hm, agn))
            lr = ds._load_and_combine_simulations(res=416, img_path=lr_paths[0], agn_path=lr_paths[1], background_path=lr_paths[2],
                                                  det_mask=masks["1x"] if masked else None)
            hr = ds._load_and_combine_simulations(res=hres, img_path=hr_paths[0], agn_path=hr_paths[1], background_path=None,
                                                  det_mask=masks[f"{hm}x"] if masked else None)
            lr, hr = normalize.normalize_lr_image(lr), normalize.normalize_hr_image(hr)
            assert lr.dtype == torch.float32 and hr.dtype == torch.float32 and lr.shape == (1, 416, 416) and hr.shape == (1, hres, hres)
            rows.append([os.path.relpath(p, tmp) for p in lr_paths + hr_paths] + [kind, str(hexp), str(hm), str(hres), str(int(masked))])
            out[f"combo{i}_lr_sha256"] = np.array(hashlib.sha256(lr.numpy().tobytes()).hexdigest())
            out[f"combo{i}_hr_sha256"] = np.array(hashlib.sha256(hr.numpy().tobytes()).hexdigest())
            out[f"combo{i}_sums"] = np.array([lr.double().sum().item(), hr.double().sum().item()])
        out["combos"] = np.array(rows)
        out["lr_max_hr_max"] = np.array([LR_MAX, HR_MAX])
        dst = os.path.join(HERE, "dataset_sim.npz")
        np.savez_compressed(dst, **out)
        print(dst, os.path.getsize(dst), "bytes")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "xmm_superres_denoise"))
