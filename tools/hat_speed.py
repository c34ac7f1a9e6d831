#!/usr/bin/env python3
"""HAT forward speed on the MI355X: the engine (csrc/hat.hip) against torch eager fp32 running the float64-oracle's restatement
(tests/golden/hat_torch.py) in fp32 on the same device, the XMM configuration (models.toml [hat]) at full depth, 416 x 416 tiles
(832 x 832 out).

  python tools/hat_speed.py time [--batches 1,4] [--iters 10] [--math fp32|bf16x6|both]
                                                                         one JSON line per batch and math mode: the median of `iters`
                                                                         event-timed forwards of both, after warm-up; with `both` the two
                                                                         modes of the engine are measured alternately, forward by forward
  python tools/hat_speed.py profile --batch 1 [--iters 3] [--math M]    engine forwards only (run under rocprofv3 --kernel-trace --stats,
                                                                         the program after `--`)
  python tools/hat_speed.py roof <kernel_stats.csv | results.db> --batch 1 --iters N [--math M] [--csv-out F]
                                                                         per-kernel time and share, achieved bytes/s against the HBM roof
                                                                         and FLOP/s against the fp32 matrix peak
  python tools/hat_speed.py counts [--batch 1]                          the per-tile FLOP and byte counts (host arithmetic)

The algorithmic bytes / FLOP of each kernel come from the shapes (every operand read once, every result written once), counted by the
code below; kernel times come from rocprofv3's own stats file.  The overlapping cross-attention is counted at its algorithmic 4 nq nk hd
FLOP per (window, head); the kernel itself computes q k^T twice (row maxima, then exp / P V), which the count does not credit.
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

import gen_hat as gh  # noqa: E402
from restormer_speed import FP32_PEAK, HBM_MEASURED, HBM_PEAK, stats_rows  # noqa: E402

CFG = gh.XMM
BF16X6_NOMINAL = 2500e12 / 6     # six bf16 MFMA products per fp32 product at the 2.5 PFLOP/s dense bf16 matrix peak: 417 TFLOP/s
GEMM_KERNEL = {"fp32": "sw_gemm_kernel", "bf16x6": "sw_gemm_s3x_kernel"}
KERNELS = ("sw_gemm_kernel", "sw_attn_kernel", "hat_ocab_kernel", "sw_ln_kernel", "hat_pool_partial_kernel", "hat_ca_kernel",
           "hat_combine_kernel")


def counts(B: int, H: int, W: int, cfg=CFG, split_gemm: bool = False, mode: str = "fp32") -> dict:
    """algorithmic {kernel: [launches, bytes, flop]} of one engine forward (fp32: 4 bytes per element); with split_gemm the GEMM's share
    is reported as its linear layers, the CAB convs and the other 3x3 convs"""
    c = gh.full_cfg(**cfg)
    E, hid, cin = c["embed_dim"], int(c["embed_dim"] * c["mlp_ratio"]), c["in_chans"]
    Cc, Cs = E // c["compress_ratio"], E // c["squeeze_factor"]
    ws, _, ow = gh.window_of(cfg)
    M = B * H * W
    nchunk = -(-H * W // 256)
    names = KERNELS + (("gemm_linear", "gemm_cab_conv", "gemm_other_conv") if split_gemm else ())
    out = {k: [0, 0.0, 0.0] for k in names}
    gk = GEMM_KERNEL[mode]           # the GEMM's counts go to the kernel that runs it (fp32 operands and results in both modes)
    out[gk] = out.pop("sw_gemm_kernel")

    def add(k, elems, flop):
        out[k][0] += 1
        out[k][1] += 4.0 * elems
        out[k][2] += float(flop)

    def gemm(rows, K, N, res=False, kind="gemm_linear"):
        add(gk, rows * K + K * N + rows * N * (2 if res else 1), 2 * rows * K * N)
        if split_gemm:
            add(kind, rows * K + K * N + rows * N * (2 if res else 1), 2 * rows * K * N)

    def ln():
        add("sw_ln_kernel", 2 * M * E, 8 * M * E)

    def mlp():
        ln()
        gemm(M, E, hid)
        gemm(M, hid, E, res=True)

    gemm(M, 9 * cin, E, kind="gemm_other_conv")           # conv_first (K = 9 taps x cin)
    ln()                                                  # patch_embed.norm
    for depth in c["depths"]:
        for _ in range(depth):
            ln()
            gemm(M, E, 3 * E)
            gemm(M, 9 * E, Cc, kind="gemm_cab_conv")
            gemm(M, 9 * Cc, E, kind="gemm_cab_conv")
            add("hat_pool_partial_kernel", M * E + 2 * B * nchunk * E, M * E)
            add("hat_ca_kernel", 2 * B * nchunk * E + 2 * E * Cs + B * E, B * (nchunk * E + 4 * E * Cs))
            add("sw_attn_kernel", 3 * M * E + M * E, 4 * M * ws * ws * E)
            gemm(M, E, E, res=True)
            add("hat_combine_kernel", 3 * M * E, 3 * M * E)
            mlp()
        ln()
        gemm(M, E, 3 * E)
        add("hat_ocab_kernel", M * E + 2 * M * E * (ow * ow) / (ws * ws) + M * E, 4 * M * ow * ow * E)
        gemm(M, E, E, res=True)
        mlp()
        if c["resi_connection"] == "1conv":
            gemm(M, 9 * E, E, res=True, kind="gemm_other_conv")
        else:
            add("hat_combine_kernel", 3 * M * E, M * E)
    ln()
    if c["resi_connection"] == "1conv":
        gemm(M, 9 * E, E, res=True, kind="gemm_other_conv")
    else:
        add("hat_combine_kernel", 3 * M * E, M * E)
    gemm(M, 9 * E, 64, kind="gemm_other_conv")
    s = c["upscale"]
    r, stages = (3, 1) if s == 3 else (2, int(math.log2(s)))
    rows = M
    for _ in range(stages):
        gemm(rows, 9 * 64, r * r * 64, kind="gemm_other_conv")
        rows *= r * r
    gemm(rows, 9 * 64, cin, kind="gemm_other_conv")
    return out


def cmd_counts(a):
    per = counts(a.batch, a.size, a.size, split_gemm=True)
    real = {k: v for k, v in per.items() if not k.startswith("gemm_")}
    tot_b, tot_f = sum(v[1] for v in real.values()), sum(v[2] for v in real.values())
    print(json.dumps({"batch": a.batch, "size": a.size, "per_kernel": {k: {"launches": v[0], "gbytes": round(v[1] / 1e9, 3),
                      "tflop": round(v[2] / 1e12, 4)} for k, v in per.items()}, "total_gbytes": round(tot_b / 1e9, 3),
                      "total_tflop": round(tot_f / 1e12, 4), "ms_at_fp32_peak": round(tot_f / FP32_PEAK * 1e3, 2)}))


def _model(math: str = "fp32"):
    import torch
    from xmm_superres_denoise.models import HAT
    state = gh.make_state(CFG, 2024)
    m = HAT(**gh.full_cfg(**CFG))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return m.set_math(math).cuda(), state


def _median_time(fn, iters):
    """median of `iters` forwards, each between its own pair of events"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        ts.append(ev0.elapsed_time(ev1) / 1e3)
    ts.sort()
    return ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]), ts[0], ts[-1]


def _alternating_times(m, x, modes, iters):
    """{mode: (median, min, max)} of `iters` forwards per mode, the modes taking turns forward by forward (same process, same clocks)"""
    import torch
    ts = {k: [] for k in modes}
    for k in modes:                  # the first forward of a mode packs its weights
        m.set_math(k)(x)
    torch.cuda.synchronize()
    for _ in range(iters):
        for k in modes:
            m.set_math(k)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            m(x)
            ev1.record()
            torch.cuda.synchronize()
            ts[k].append(ev0.elapsed_time(ev1) / 1e3)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), v[0], v[-1])
    return out


def cmd_time(a):
    import torch
    import hat_torch as ht
    modes = ["fp32", "bf16x6"] if a.math == "both" else [a.math]
    m, state = _model(modes[0])
    sd = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
    tflop = sum(v[2] for v in counts(1, a.size, a.size).values()) / 1e12
    gemm_tflop = counts(1, a.size, a.size)["sw_gemm_kernel"][2] / 1e12
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.from_numpy(gh.make_input((B, 1, a.size, a.size), 7)).cuda()
        with torch.no_grad():
            for _ in range(2):          # warm-up: workspace plan, code objects, library algorithm choices
                m(x)
                ht.hat_forward(sd, x, **CFG)
            eng = _alternating_times(m, x, modes, a.iters)
            t_eager, lo_t, hi_t = _median_time(lambda: ht.hat_forward(sd, x, **CFG), a.iters)
            y_eager = ht.hat_forward(sd, x, **CFG)
            dmaxs = {k: float((m.set_math(k)(x) - y_eager).abs().max()) for k in modes}
        for k in modes:
            t_eng, lo_e, hi_e = eng[k]
            dmax = dmaxs[k]
            print(json.dumps({"model": "hat", "math": k, "batch": B, "size": a.size, "iters": a.iters, "engine_ms": round(t_eng * 1e3, 3),
                              "engine_ms_min_max": [round(lo_e * 1e3, 3), round(hi_e * 1e3, 3)],
                              "engine_images_per_s": round(B / t_eng, 3), "torch_eager_fp32_ms": round(t_eager * 1e3, 3),
                              "torch_eager_fp32_ms_min_max": [round(lo_t * 1e3, 3), round(hi_t * 1e3, 3)],
                              "torch_eager_fp32_images_per_s": round(B / t_eager, 3), "engine_over_eager": round(t_eager / t_eng, 3),
                              "algorithmic_tflop_per_image": round(tflop, 3), "engine_tflops": round(B * tflop / t_eng, 2),
                              "share_of_fp32_matrix_peak": round(B * tflop * 1e12 / t_eng / FP32_PEAK, 4),
                              "share_of_bf16x6_nominal": round(B * tflop * 1e12 / t_eng / BF16X6_NOMINAL, 4),
                              "gemm_tflop_per_image": round(gemm_tflop, 3),
                              "max_abs_diff": dmax, "device": torch.cuda.get_device_name(0)}), flush=True)


def cmd_profile(a):
    import torch
    m, _ = _model(a.math)
    x = torch.from_numpy(gh.make_input((a.batch, 1, a.size, a.size), 7)).cuda()
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
    agg = {}
    for r in rows:
        name = r.get("Name", r.get("KernelName", ""))
        key = next((k for k in per if k in name), None)
        if key is None:
            continue
        a_ = agg.setdefault(key, [0, 0.0])
        a_[0] += int(float(r["Calls"]))
        a_[1] += float(r["TotalDurationNs"]) * 1e-9
    all_s = sum(v[1] for v in agg.values())
    print(f"# kernel, calls, total ms, ms per forward, share of the kernel time, GB/s achieved, share of 8.0 TB/s (of 6.3 measured), GFLOP/s, "
          f"share of 157 TF/s, share of the 417 TF/s bf16x6 nominal; math {a.math}, B = {a.batch}, {a.size} x {a.size}, {n_fwd} forwards")
    for key, (calls, tot_s) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        launches, nbytes, flop = per[key]
        bps, fps = nbytes * n_fwd / tot_s, flop * n_fwd / tot_s
        print(f"{key}, {calls} (expected {launches * n_fwd}), {tot_s * 1e3:.3f}, {tot_s * 1e3 / n_fwd:.3f}, {tot_s / all_s:.4f}, {bps / 1e9:.0f}, "
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
