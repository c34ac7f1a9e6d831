#!/usr/bin/env python3
"""SwinIR TRAIN-step speed on the MI355X: TrainableSwinIR (models/modules/swinir_train.py: the differentiable HIP ops of
xmm_superres_denoise/ops.py under torch's autograd) against torch eager autograd of the restatement tests/golden/swinir_torch.py in fp32,
on the same device, in the same process, the two taking turns step by step.  One step = forward, L1 loss, backward, Adam
(torch.optim.Adam in both).  Denoising head, B = 1, a native 403 x 411 detector image (reflect-padded to 408 x 416), window 8.

  python tools/swinir_train_speed.py [--work mid,full] [--iters 5] [--groups N]
      mid    embed_dim 60, depths [4] x 2, 6 heads
      full   embed_dim 180, depths [6] x 6 (or [6] x N with --groups N), 6 heads: the full-depth denoiser
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

import gen_swinir as gi  # noqa: E402
import swinir_torch as sit  # noqa: E402

SHAPE = (1, 1, 403, 411)


def work(name: str, groups: int) -> dict:
    base = dict(img_size=64, patch_size=1, in_chans=1, window_size=8, upscale=1, upsampler="", drop_path_rate=0.0)
    if name == "mid":
        return dict(base, embed_dim=60, depths=[4] * 2, num_heads=[6] * 2)
    return dict(base, embed_dim=180, depths=[6] * groups, num_heads=[6] * groups)


def run(name: str, cfg: dict, iters: int) -> dict:
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    dev = torch.device("cuda:0")
    state = gi.make_state(cfg, 7)
    m = SwinIR(**gi.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    net = TrainableSwinIR(m.to(dev)).train()
    names = {k for k, _ in m.named_parameters()}
    sd = {k: (v.detach().clone().requires_grad_(True) if k in names else v.detach()) for k, v in m.state_dict().items()}
    x = torch.from_numpy(gi.make_input(SHAPE, 8)).to(dev)
    t = torch.from_numpy(gi.make_input(SHAPE, 9)).to(dev)
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
        loss = F.l1_loss(sit.swinir_forward(sd, x, **cfg), t)
        loss.backward()
        opt_t.step()
        return loss

    steps = {"engine": step_engine, "eager": step_eager}
    peak, first = {}, {}
    for k, fn in steps.items():                      # warm-up, and the peak memory of one step on its own
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        first[k] = float(fn())
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
    out = {"tool": "swinir_train_speed", "work": name, "cfg": {k: cfg[k] for k in ("embed_dim", "depths", "num_heads", "window_size")},
           "shape": list(SHAPE), "iters": iters, "first_loss": first}
    for k in steps:
        out[k] = {"ms_median": round(statistics.median(times[k]), 3), "ms_min": round(min(times[k]), 3), "ms_max": round(max(times[k]), 3),
                  "peak_mib": round(peak[k], 1)}
    out["engine_over_eager"] = round(out["engine"]["ms_median"] / out["eager"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="mid,full")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--groups", type=int, default=6, help="RSTB groups of the full workload (6 = full depth)")
    ap.add_argument("--one-step", action="store_true", help="one engine step of each workload and nothing else (for a kernel-stats run)")
    a = ap.parse_args()
    for name in a.work.split(","):
        cfg = work(name, a.groups)
        if a.one_step:
            from xmm_superres_denoise.train import fit_swinir
            fit_swinir(gi.full_cfg(**cfg), steps=2, batch_size=1, lr_res=408, log_every=0)
            torch.cuda.synchronize()
            continue
        print(json.dumps(run(name, cfg, a.iters)), flush=True)


if __name__ == "__main__":
    main()
