#!/usr/bin/env python3
"""Generate the SwinIR golden fixtures from the REFERENCE's own module.

Runs only where a checkout of the reference is available (its root is the one argument).  As make_golden_swinfir.py does, this script
puts a small stand-in timm (timm, timm.layers, timm.models.layers: trunc_normal_ and to_2tuple, which is all the transformer package
takes from timm) and empty `models` / `models.transformer` packages into sys.modules and loads the reference's tools.py, modules.py and
swinir.py by path.  No reference source is copied and no weights are stored: weights and inputs are regenerated from
gen_swinir.make_state / make_input (numpy PCG64, state-dict order).

Outputs (committed, each <= 2 MB):
  swinir_<case>.npz   x, the reference's fp32 output y32 and its float64 output y64 (`.double()` module and input), cfg, seed
  swinir_keys.npz     names and shapes of the state_dict of case a's configuration widened to embed_dim 60 (6 heads), and per-tensor sums
                      of its default initialisation under torch.manual_seed(0)

usage: python tests/golden/make_golden_swinir.py <reference checkout root>
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_swinir as gi  # noqa: E402
from make_golden_swinfir import _stub_timm  # noqa: E402

KEYS_CFG = dict(gi.CASES["a_dn_reflect"]["cfg"], embed_dim=60, num_heads=[6, 6])


def import_reference_swinir(root):
    import importlib.util
    import types
    _stub_timm()
    for name in ("models", "models.transformer"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    d = os.path.join(root, "xmm_superres_denoise", "models", "transformer")
    for mod in ("tools", "modules", "swinir"):
        spec = importlib.util.spec_from_file_location(f"models.transformer.{mod}", os.path.join(d, mod + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
    return sys.modules["models.transformer.swinir"].SwinIR


def main(root):
    SwinIR = import_reference_swinir(root)
    torch.manual_seed(0)
    m = SwinIR(**gi.full_cfg(**KEYS_CFG))
    sd = m.state_dict()
    names, shapes = list(sd.keys()), [tuple(v.shape) for v in sd.values()]
    mine = gi.param_shapes(KEYS_CFG)
    assert list(mine.keys()) == names and list(mine.values()) == shapes, "gen_swinir.param_shapes disagrees with the reference"
    init = np.array([[v.double().sum().item(), (v.double() ** 2).sum().item()] for v in sd.values()])
    nparams = sum(p.numel() for p in m.parameters())
    np.savez_compressed(os.path.join(HERE, "swinir_keys.npz"), names=np.array(names), shapes=np.array(json.dumps(shapes)),
                        nparams=np.int64(nparams), init_seed0=init, cfg=np.array(json.dumps(KEYS_CFG)))
    print(f"keys: {len(names)} tensors, {nparams} parameters")
    for case, spec in gi.CASES.items():
        m = SwinIR(**gi.full_cfg(**spec["cfg"])).eval()
        state = gi.make_state(spec["cfg"], spec["seed"])
        ref_sd = m.state_dict()
        assert list(ref_sd.keys()) == list(state.keys()), case
        for k, v in state.items():
            assert tuple(ref_sd[k].shape) == v.shape, (case, k)
            if k.endswith("index") or k.endswith("mask"):
                assert np.array_equal(ref_sd[k].numpy(), v), (case, k)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        x = gi.make_input(spec["shape"], spec["seed"] + 1000)
        with torch.no_grad():
            y32 = m(torch.from_numpy(x)).numpy()
            y64 = m.double()(torch.from_numpy(x).double()).numpy()
        out = os.path.join(HERE, f"swinir_{case}.npz")
        np.savez_compressed(out, x=x, y32=y32, y64=y64, cfg=np.array(json.dumps(spec["cfg"])), seed=np.int64(spec["seed"]))
        err = np.abs(y32 - y64)
        print(f"{case}: {os.path.getsize(out)} B, out {y64.shape}, fp32 vs float64 rms {np.sqrt((err ** 2).mean()):.3e} "
              f"max {err.max():.3e} (|y| max {np.abs(y64).max():.3f})")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
