#!/usr/bin/env python3
"""Generate the Restormer golden fixtures past 64 channels per head from the REFERENCE's own module.

Runs only where a checkout of the reference is available (its root is the one argument); the reference's restormer.py is imported by
path, as make_golden_restormer.py does.  No reference source is copied and no weights are stored: weights and inputs are regenerated
from gen_restormer.make_state / make_input (numpy PCG64, state-dict order).

Outputs (committed, a few KB each):
  restormer_<case>.npz      x, the reference's fp32 output y32 and its float64 output y64 (`.double()` module and input), the
                            constructor arguments `cfg` (JSON) and the `seed`, for the cases of gen_restormer_wide.CASES
  restormer_keys_dim48.npz  names and shapes of Restormer().state_dict() (the class defaults, restormer.py:218-230: the network as
                            published) and per-tensor sums of its default initialisation under torch.manual_seed(0)

usage: python tests/golden/make_golden_restormer_wide.py <reference checkout root>
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_restormer_wide as gw  # noqa: E402


def import_reference_restormer(root):
    path = os.path.join(root, "xmm_superres_denoise", "models", "transformer", "restormer.py")
    spec = importlib.util.spec_from_file_location("_ref_restormer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Restormer


def main(root):
    Restormer = import_reference_restormer(root)
    torch.manual_seed(0)
    sd = Restormer().state_dict()
    names, shapes = list(sd.keys()), [tuple(v.shape) for v in sd.values()]
    mine = gw.param_shapes({})
    assert list(mine.keys()) == names and list(mine.values()) == shapes, "gen_restormer.param_shapes disagrees with the reference"
    # default initialisation under torch.manual_seed(0): per-tensor sum and sum of squares (float64)
    init = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    np.savez_compressed(os.path.join(HERE, "restormer_keys_dim48.npz"), names=np.array(names),
                        shapes=np.array(json.dumps(shapes)), nparams=np.int64(sum(v.numel() for v in sd.values())), init_seed0=init)
    print(f"keys: {len(names)} tensors, {sum(v.numel() for v in sd.values())} parameters")
    for case, spec in gw.CASES.items():
        m = Restormer(**gw.full_cfg(**spec["cfg"])).eval()
        state = gw.make_state(spec["cfg"], spec["seed"])
        ref_sd = m.state_dict()
        assert list(ref_sd.keys()) == list(state.keys()), case
        for k, v in state.items():
            assert tuple(ref_sd[k].shape) == v.shape, (case, k)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        x = gw.make_input(spec["shape"], spec["seed"] + 1000)
        with torch.no_grad():
            y32 = m(torch.from_numpy(x)).numpy()
            y64 = m.double()(torch.from_numpy(x).double()).numpy()
        out = os.path.join(HERE, f"restormer_{case}.npz")
        np.savez_compressed(out, x=x, y32=y32, y64=y64, cfg=np.array(json.dumps(spec["cfg"])), seed=np.int64(spec["seed"]))
        err = np.abs(y32 - y64)
        print(f"{case}: {os.path.getsize(out)} B, fp32 vs float64 rms {np.sqrt((err ** 2).mean()):.3e} max {err.max():.3e} "
              f"(|y| max {np.abs(y64).max():.3f})")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
