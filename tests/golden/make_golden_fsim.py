"""Writes tests/golden/fsim_cases.npz: float64 values of the plain-torch restatement of fsim (fsim_torch.py) on the seeded photon-like
pairs of the GPU accuracy test (tests/test_hip_fsim.py), so that a later edit of the restatement cannot drift silently.  The inputs are
not stored: `fsim_torch.case_pair` regenerates them from the seeds (tests/test_fsim_host.py does the same and compares); stored per case
are the inputs' checksums, the per-image fsim and its two sums (numerator, sum of pc_max).

    python tests/golden/make_golden_fsim.py
"""
import os

import numpy as np

import fsim_torch as Fs

HERE = os.path.dirname(os.path.abspath(__file__))


def values(p, t):
    num, den = Fs.fsim_parts(p.double(), t.double())
    return {"fsim": (num / den).numpy(), "num": num.numpy(), "pc_max_sum": den.numpy()}


def main():
    z = {}
    for name in Fs.CASES:
        p, t = Fs.case_pair(name)
        z[name + "/checksum"] = np.array([p.double().sum().item(), t.double().sum().item()])
        for k, v in values(p, t).items():
            z[f"{name}/{k}"] = v
    np.savez(os.path.join(HERE, "fsim_cases.npz"), **z)
    print("wrote fsim_cases.npz:", len(z), "arrays")


if __name__ == "__main__":
    main()
