#!/usr/bin/env python3
"""HAT TRAIN-step speed on the MI355X: TrainableHAT (models/modules/hat_train.py: the differentiable HIP ops of
xmm_superres_denoise/ops.py, overlap_attention and channel_attention among them, under torch's autograd) against torch eager autograd
of the restatement tests/golden/hat_torch.py in fp32, on the same device, in the same process, the two taking turns step by step.  One
step = forward, L1 loss, backward, Adam (torch.optim.Adam in both), B = 1, x2 pixelshuffle, resi_connection "1conv".

  python tools/hat_train_speed.py [--work mid,full] [--iters 5] [--groups N] [--depth D]
      mid    embed_dim 60, depths [4] x 2, 6 heads, window 8 (overlap window 12), a 64 x 64 tile
      full   the [hat] configuration of models.toml (embed_dim 180, depths [6] x 6, 6 heads, window 16, overlap window 24) on a
             416 x 416 tile; --groups N with --depth D takes [D] x N.  If a step runs out of memory the tool says so and exits with
             status 2: run it again with half the groups (the line's "cfg" shows the depths that were timed)
      one JSON line per workload: medians of `iters` event-timed steps after one warm-up step each, with [min, max], and the peak
      memory of one step of each (torch.cuda.max_memory_allocated)
This number is recorded, not gated.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gen_hat as gs  # noqa: E402
import hat_torch as st  # noqa: E402


def work(name: str, groups: int, depth: int):
    if name == "mid":
        return dict(img_size=64, patch_size=1, in_chans=1, window_size=8, upscale=2, upsampler="pixelshuffle", drop_path_rate=0.0,
                    resi_connection="1conv", embed_dim=60, depths=[4] * 2, num_heads=[6] * 2), (1, 1, 64, 64)
    return dict(gs.XMM, drop_path_rate=0.0, resi_connection="1conv", depths=[depth] * groups, num_heads=[6] * groups), (1, 1, 416, 416)


def run(name: str, cfg: dict, shape, iters: int) -> dict:
    from xmm_superres_denoise.models import HAT, TrainableHAT
    dev = torch.device("cuda:0")
    state = gs.make_state(cfg, 7)
    m = HAT(**gs.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    net = TrainableHAT(m.to(dev)).train()
    names = {k for k, _ in m.named_parameters()}
    sd = {k: (v.detach().clone().requires_grad_(True) if k in names else v.detach()) for k, v in m.state_dict().items()}
    x = torch.from_numpy(gs.make_input(shape, 8)).to(dev)
    t = torch.from_numpy(gs.make_input((shape[0], shape[1], 2 * shape[2], 2 * shape[3]), 9)).to(dev)
    opt_e = torch.optim.Adam(list(net.parameters()), lr=2e-4)
    opt_t = torch.optim.Adam([v for v in sd.values() if v.requires_grad], lr=2e-4)

    def step_engine():
        opt_e.zero_grad(set_to_none=True)
        loss = F.l1_loss(net(x), t)
        loss.backward()
        opt_e.step()
        return loss

    def step_eager():
        opt_t.zero_grad(set_to_none=True)
        loss = F.l1_loss(st.hat_forward(sd, x, **cfg), t)
        loss.backward()
        opt_t.step()
        return loss

    steps = {"engine": step_engine, "eager": step_eager}
    peak, first = {}, {}
    for k, fn in steps.items():                      # warm-up, and the peak memory of one step on its own
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        first[k] = float(fn().detach())
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() / 2 ** 20
    times = {k: [] for k in steps}
    for _ in range(iters):
        for k, fn in steps.items():                  # alternately: both see the same clocks and the same neighbours
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    out = {"tool": "hat_train_speed", "work": name, "cfg": {k: cfg[k] for k in ("embed_dim", "depths", "num_heads", "window_size", "resi_connection")},
           "window": m.window, "shape": list(shape), "iters": iters, "first_loss": first}
    for k in steps:
        out[k] = {"ms_median": round(statistics.median(times[k]), 3), "ms_min": round(min(times[k]), 3), "ms_max": round(max(times[k]), 3),
                  "peak_mib": round(peak[k], 1)}
    out["engine_over_eager"] = round(out["engine"]["ms_median"] / out["eager"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="mid,full")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--groups", type=int, default=6, help="RHAGs of the full workload (6 = full depth)")
    ap.add_argument("--depth", type=int, default=6, help="HABs per RHAG of the full workload (6 = full depth)")
    a = ap.parse_args()
    for name in a.work.split(","):
        cfg, shape = work(name, a.groups, a.depth)
        try:
            out = run(name, cfg, shape, a.iters)
        except torch.cuda.OutOfMemoryError:      # no second run in this process: the caller starts one, under its own time limit
            print(json.dumps({"tool": "hat_train_speed", "work": name, "error": f"out of memory with {a.groups} groups; run again "
                                                                                      f"with --groups {max(1, a.groups // 2)}"}), flush=True)
            sys.exit(2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
