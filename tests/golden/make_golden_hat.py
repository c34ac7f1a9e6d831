#!/usr/bin/env python3
"""Generate the HAT golden fixtures from the REFERENCE's own module.

Runs only where a checkout of the reference is available (its root is the one argument).  As in make_golden_swinfir.py, a small stand-in
timm (only trunc_normal_ and to_2tuple are used; timm's trunc_normal_ is the same draw as torch.nn.init.trunc_normal_) and empty
`models` / `models.transformer` packages go into sys.modules, and the reference's tools.py, modules.py and hat.py are loaded by path
(hat.py also imports einops, which must be installed).  No reference source is copied and no weights are stored: weights and inputs are
regenerated from gen_hat.make_state / make_input (numpy PCG64, state-dict order).

Outputs (committed, each <= 2 MB):
  hat_<case>.npz     x, the reference's fp32 output y32 and its float64 output y64 (`.double()` module and input), cfg, seed
  hat_keys_xmm.npz   names and shapes of the XMM configuration's state_dict (models.toml [hat] through model.py:216-229), its parameter
                     count, and per-tensor sums of its default initialisation under torch.manual_seed(0)

usage: python tests/golden/make_golden_hat.py <reference checkout root>
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_hat as gh  # noqa: E402
from make_golden_swinfir import _stub_timm  # noqa: E402


def import_reference_hat(root):
    _stub_timm()
    for name in ("models", "models.transformer"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    d = os.path.join(root, "xmm_superres_denoise", "models", "transformer")
    for mod in ("tools", "modules", "hat"):
        spec = importlib.util.spec_from_file_location(f"models.transformer.{mod}", os.path.join(d, mod + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
    return sys.modules["models.transformer.hat"].HAT


def main(root):
    HAT = import_reference_hat(root)
    torch.manual_seed(0)
    m = HAT(**gh.full_cfg(**gh.XMM))
    sd = m.state_dict()
    names, shapes = list(sd.keys()), [tuple(v.shape) for v in sd.values()]
    mine = gh.param_shapes(gh.XMM)
    assert list(mine.keys()) == names and list(mine.values()) == shapes, "gen_hat.param_shapes disagrees with the reference"
    init = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    nparams = sum(p.numel() for p in m.parameters())
    np.savez_compressed(os.path.join(HERE, "hat_keys_xmm.npz"), names=np.array(names), shapes=np.array(json.dumps(shapes)),
                        nparams=np.int64(nparams), init_seed0=init)
    print(f"keys: {len(names)} tensors, {nparams} parameters")
    for case, spec in gh.CASES.items():
        m = HAT(**gh.full_cfg(**spec["cfg"])).eval()
        state = gh.make_state(spec["cfg"], spec["seed"])
        ref_sd = m.state_dict()
        assert list(ref_sd.keys()) == list(state.keys()), case
        for k, v in state.items():
            assert tuple(ref_sd[k].shape) == v.shape, (case, k)
            if k.startswith("relative_position_index"):
                assert np.array_equal(ref_sd[k].numpy(), v), (case, k)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        x = gh.make_input(spec["shape"], spec["seed"] + 1000)
        with torch.no_grad():
            y32 = m(torch.from_numpy(x)).numpy()
            y64 = m.double()(torch.from_numpy(x).double()).numpy()
        out = os.path.join(HERE, f"hat_{case}.npz")
        np.savez_compressed(out, x=x, y32=y32, y64=y64, cfg=np.array(json.dumps(spec["cfg"])), seed=np.int64(spec["seed"]))
        err = np.abs(y32 - y64)
        print(f"{case}: {os.path.getsize(out)} B, out {y64.shape}, fp32 vs float64 rms {np.sqrt((err ** 2).mean()):.3e} "
              f"max {err.max():.3e} (|y| max {np.abs(y64).max():.3f})")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
