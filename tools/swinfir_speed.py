#!/usr/bin/env python3
"""SwinFIR forward speed on the MI355X: the engine (csrc/swinfir.hip) against torch eager fp32 running the float64-oracle's
restatement (tests/golden/swinfir_torch.py) in fp32 on the same device, the XMM configuration (models.toml [swinfir]), 416 x 416 tiles
(832 x 832 out).

  python tools/swinfir_speed.py time [--batches 1,4] [--iters 10] [--math fp32|bf16x6|both]
                                                                     one JSON line per batch and math mode: images/s of both; with
                                                                     `both` the engine's two modes are measured alternately, forward by
                                                                     forward
  python tools/swinfir_speed.py profile --batch 1 [--iters 3] [--math M]    engine forwards only (run under rocprofv3 --kernel-trace --stats)
  python tools/swinfir_speed.py roof <kernel_stats.csv | results.db> --batch 1 --iters N [--math M] [--csv-out F]
                                                                     per-kernel time, achieved bytes/s against the HBM roof and
                                                                     FLOP/s against the fp32 peak
  python tools/swinfir_speed.py counts [--batch 1]                          the per-tile FLOP and byte counts (host arithmetic)

The algorithmic bytes / FLOP of each kernel come from the shapes (every operand read once, every result written once; an FFT line of
n points counted as 5 n log2 n FLOP), counted by the code below; kernel times come from rocprofv3's own stats file.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_swinfir as gs  # noqa: E402
from hat_speed import BF16X6_NOMINAL, GEMM_KERNEL, _alternating_times  # noqa: E402
from restormer_speed import FP32_PEAK, HBM_MEASURED, HBM_PEAK, _time, stats_rows  # noqa: E402

CFG = gs.XMM
KERNELS = ("sw_gemm_kernel", "sw_attn_kernel", "sw_fft_kernel", "sw_ln_kernel")


def counts(B: int, H: int, W: int, cfg=CFG, mode: str = "fp32") -> dict:
    """algorithmic {kernel: [launches, bytes, flop]} of one engine forward (fp32: 4 bytes per element)"""
    c = gs.full_cfg(**cfg)
    E, hid, C2, cin = c["embed_dim"], int(c["embed_dim"] * c["mlp_ratio"]), c["embed_dim"] // 2, c["in_chans"]
    ws, _, _ = gs.window_of(cfg)
    M, Wk = B * H * W, W // 2 + 1
    Ms = B * H * Wk
    out = {k: [0, 0.0, 0.0] for k in KERNELS}
    gk = GEMM_KERNEL[mode]           # the GEMM's counts go to the kernel that runs it (fp32 operands and results in both modes)
    out[gk] = out.pop("sw_gemm_kernel")

    def add(k, elems, flop):
        out[k][0] += 1
        out[k][1] += 4.0 * elems
        out[k][2] += float(flop)

    def gemm(rows, K, N, res=False):
        add(gk, rows * K + K * N + rows * N * (2 if res else 1), 2 * rows * K * N)

    def fft(lines, n, complex_in, complex_out):
        add("sw_fft_kernel", lines * n * ((2 if complex_in else 1) + (2 if complex_out else 1)), 5 * lines * n * math.log2(n))

    gemm(M, 9 * cin, E)                                   # conv_first (K = 9 taps x cin)
    add("sw_ln_kernel", 2 * M * E, 8 * M * E)             # patch_embed.norm
    for depth in c["depths"]:
        for _ in range(depth):
            add("sw_ln_kernel", 2 * M * E, 8 * M * E)
            gemm(M, E, 3 * E)
            add("sw_attn_kernel", 3 * M * E + M * E, 4 * M * ws * ws * E)
            gemm(M, E, E, res=True)
            add("sw_ln_kernel", 2 * M * E, 8 * M * E)
            gemm(M, E, hid)
            gemm(M, hid, E, res=True)
        if c["resi_connection"] == "SFB":
            gemm(M, 9 * E, E)
            gemm(M, 9 * E, E, res=True)
            gemm(M, E, C2)
            fft(B * H * C2, W, False, True)
            fft(B * Wk * C2, H, True, True)
            gemm(Ms, 2 * C2, 2 * C2)
            fft(B * Wk * C2, H, True, True)
            fft(B * H * C2, W, True, False)
            gemm(M, C2, E)
            gemm(M, 2 * E, E, res=True)
        else:
            gemm(M, 9 * E, E, res=True)
    add("sw_ln_kernel", 2 * M * E, 8 * M * E)
    gemm(M, 9 * E, E, res=True)
    gemm(M, 9 * E, 64)
    s = c["upscale"]
    r, stages = (3, 1) if s == 3 else (2, int(math.log2(s)))
    rows = M
    for _ in range(stages):
        gemm(rows, 9 * 64, r * r * 64)
        rows *= r * r
    gemm(rows, 9 * 64, cin)
    return out


def cmd_counts(a):
    per = counts(a.batch, a.size, a.size)
    tot_b, tot_f = sum(v[1] for v in per.values()), sum(v[2] for v in per.values())
    print(json.dumps({"batch": a.batch, "size": a.size, "per_kernel": {k: {"launches": v[0], "gbytes": round(v[1] / 1e9, 3),
                      "tflop": round(v[2] / 1e12, 4)} for k, v in per.items()}, "total_gbytes": round(tot_b / 1e9, 3),
                      "total_tflop": round(tot_f / 1e12, 4), "ms_at_fp32_peak": round(tot_f / FP32_PEAK * 1e3, 2)}))


def _model(math: str = "fp32"):
    import torch
    from xmm_superres_denoise.models import SwinFIR
    state = gs.make_state(CFG, 2024)
    m = SwinFIR(**gs.full_cfg(**CFG))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return m.set_math(math).cuda(), state


def cmd_time(a):
    import numpy as np
    import torch
    import swinfir_torch as st
    modes = ["fp32", "bf16x6"] if a.math == "both" else [a.math]
    m, state = _model(modes[0])
    tflop = sum(v[2] for v in counts(1, a.size, a.size).values()) / 1e12
    sd = {k: torch.from_numpy(v).cuda() if v.dtype == np.float32 else torch.from_numpy(v).cuda() for k, v in state.items()}
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.from_numpy(gs.make_input((B, 1, a.size, a.size), 7)).cuda()
        with torch.no_grad():
            for _ in range(2):          # warm-up: workspace plan, code objects, library algorithm choices
                m(x)
                st.swinfir_forward(sd, x, **CFG)
            eng = _alternating_times(m, x, modes, a.iters)
            t_eager = _time(lambda: st.swinfir_forward(sd, x, **CFG), a.iters)
            y_eager = st.swinfir_forward(sd, x, **CFG)
            dmaxs = {k: float((m.set_math(k)(x) - y_eager).abs().max()) for k in modes}
        for k in modes:
            t_eng, lo_e, hi_e = eng[k]
            print(json.dumps({"model": "swinfir", "math": k, "batch": B, "size": a.size, "iters": a.iters, "engine_ms": round(t_eng * 1e3, 3),
                              "engine_ms_min_max": [round(lo_e * 1e3, 3), round(hi_e * 1e3, 3)],
                              "engine_images_per_s": round(B / t_eng, 2), "torch_eager_fp32_ms": round(t_eager * 1e3, 3),
                              "torch_eager_fp32_images_per_s": round(B / t_eager, 2), "engine_over_eager": round(t_eager / t_eng, 3),
                              "share_of_fp32_matrix_peak": round(B * tflop * 1e12 / t_eng / FP32_PEAK, 4),
                              "share_of_bf16x6_nominal": round(B * tflop * 1e12 / t_eng / BF16X6_NOMINAL, 4),
                              "max_abs_diff": dmaxs[k], "device": torch.cuda.get_device_name(0)}), flush=True)


def cmd_profile(a):
    import torch
    m, _ = _model(a.math)
    x = torch.from_numpy(gs.make_input((a.batch, 1, a.size, a.size), 7)).cuda()
    with torch.no_grad():
        m(x)            # first forward: plan + pack (the stats file counts it: `roof` takes iters + 1 forwards)
        for _ in range(a.iters):
            m(x)
    torch.cuda.synchronize()
    print(json.dumps({"profiled_forwards": a.iters + 1, "math": a.math, "batch": a.batch, "size": a.size}))


def cmd_roof(a):
    import csv
    per = counts(a.batch, a.size, a.size, mode=a.math)
    n_fwd = a.iters + 1
    rows = stats_rows(a.stats)
    if a.csv_out:
        with open(a.csv_out, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage"], extrasaction="ignore")
            w.writeheader()
            w.writerows(rows)
    print(f"# kernel, calls, total ms, ms per forward, GB/s achieved, share of 8.0 TB/s (of 6.3 measured), GFLOP/s, share of 157 TF/s, share of the 417 TF/s bf16x6 nominal; "
          f"math {a.math}, B = {a.batch}, {a.size} x {a.size}, {n_fwd} forwards")
    agg = {}
    for r in rows:
        name = r.get("Name", r.get("KernelName", ""))
        key = next((k for k in per if k in name), None)
        if key is None:
            continue
        a_ = agg.setdefault(key, [0, 0.0])
        a_[0] += int(float(r["Calls"]))
        a_[1] += float(r["TotalDurationNs"]) * 1e-9
    for key, (calls, tot_s) in agg.items():
        launches, nbytes, flop = per[key]
        bps, fps = nbytes * n_fwd / tot_s, flop * n_fwd / tot_s
        print(f"{key}, {calls} (expected {launches * n_fwd}), {tot_s * 1e3:.3f}, {tot_s * 1e3 / n_fwd:.3f}, {bps / 1e9:.0f}, "
              f"{bps / HBM_PEAK:.3f} ({bps / HBM_MEASURED:.3f}), {fps / 1e9:.0f}, {fps / FP32_PEAK:.4f}, {fps / BF16X6_NOMINAL:.4f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--batches", default="1,4")
    t.add_argument("--iters", type=int, default=10)
    t.add_argument("--size", type=int, default=416)
    t.add_argument("--math", default="fp32", choices=["fp32", "bf16x6", "both"])
    p = sub.add_parser("profile")
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--size", type=int, default=416)
    p.add_argument("--math", default="fp32", choices=["fp32", "bf16x6"])
    r = sub.add_parser("roof")
    r.add_argument("stats")
    r.add_argument("--batch", type=int, default=1)
    r.add_argument("--iters", type=int, default=3)
    r.add_argument("--size", type=int, default=416)
    r.add_argument("--math", default="fp32", choices=["fp32", "bf16x6"])
    r.add_argument("--csv-out", default=None, help="also write the kernel stats as CSV")
    c = sub.add_parser("counts")
    c.add_argument("--batch", type=int, default=1)
    c.add_argument("--size", type=int, default=416)
    a = ap.parse_args()
    {"time": cmd_time, "profile": cmd_profile, "roof": cmd_roof, "counts": cmd_counts}[a.cmd](a)


if __name__ == "__main__":
    main()
