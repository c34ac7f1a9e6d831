"""Writes tests/golden/ext_metrics_cases.npz: float64 values of the plain-torch restatement of the extended test metrics
(ext_metrics_torch.py) on seeded inputs, so that a later edit of the restatement cannot drift silently.  The inputs are not
stored: `cases()` regenerates them from the seeds (tests/test_ext_metrics_host.py does the same and compares).

    python tests/golden/make_golden_ext_metrics.py
"""
import os

import numpy as np
import torch

import ext_metrics_torch as E

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("a_96x96", (2, 96, 96), 11), ("b_61x53", (2, 61, 53), 12), ("c_130x77", (1, 130, 77), 13), ("d_41x41", (1, 41, 41), 14))


def cases():
    """name -> (preds, target) float64 [B, H, W]"""
    out = {}
    for name, shape, seed in CASES:
        out[name] = E.photon_pair(shape, torch.Generator().manual_seed(seed))
    return out


def values(p, t):
    v = {n: f(p, t).numpy() for n, f in E.FUNCS.items()}
    v["ms_gmsd_scales"] = E.ms_gmsd_scales(p, t).numpy()
    v["mdsi_deviation"] = E.mdsi_deviation(p, t).numpy()
    v["vif_num"], v["vif_den"] = (a.numpy() for a in E.vif_parts(p, t))
    v["haarpsi_num"], v["haarpsi_den"] = (a.numpy() for a in E.haarpsi_parts(p, t))
    return v


def main():
    z = {}
    for name, (p, t) in cases().items():
        z[name + "/checksum"] = np.array([p.sum().item(), t.sum().item()])
        for k, v in values(p, t).items():
            z[f"{name}/{k}"] = v
    np.savez(os.path.join(HERE, "ext_metrics_cases.npz"), **z)
    print("wrote ext_metrics_cases.npz:", len(z), "arrays")


if __name__ == "__main__":
    main()
