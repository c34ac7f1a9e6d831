#!/usr/bin/env python3
"""SwinIR forward speed on the MI355X: the engine (csrc/swinir.hip) against torch eager fp32 running the restatement
(tests/golden/swinir_torch.py) in fp32 on the same device and in the same process.  Two workloads on one body (embed 180, 6 x 6 blocks
of 6 heads, window 8, "1conv"):
  dn   the denoising head (upsampler "", upscale 1) on a native 403 x 411 detector image, reflect-padded to 408 x 416 inside the engine
  sr   the classical head ("pixelshuffle", upscale 2) on 416 x 416 tiles (832 x 832 out)

  python tools/swinir_speed.py time [--work dn,sr] [--batches 1,4] [--iters 10] [--math fp32|bf16x6|both]
                                      one JSON line per workload, batch and math mode (dn runs at B = 1 only): medians of `iters`
                                      event-timed forwards after warm-up, with [min, max]; with `both` the engine's two modes take turns
                                      forward by forward
  python tools/swinir_speed.py counts [--work dn] [--batch 1]
                                      the algorithmic FLOP and bytes per kernel of one forward (host arithmetic: every operand read
                                      once, every result written once) and the time they take at the fp32 matrix peak and the HBM roof
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

import gen_swinir as gi  # noqa: E402
from hat_speed import BF16X6_NOMINAL, GEMM_KERNEL, _alternating_times  # noqa: E402
from restormer_speed import FP32_PEAK, HBM_PEAK  # noqa: E402

BODY = dict(img_size=64, patch_size=1, in_chans=1, embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, window_size=8)
WORK = {"dn": (dict(BODY, upscale=1, upsampler=""), (403, 411)),
        "sr": (dict(BODY, upscale=2, upsampler="pixelshuffle"), (416, 416))}
KERNELS = ("sw_gemm_kernel", "sw_attn_kernel", "sw_ln_kernel", "swinir_pad_kernel")


def counts(B: int, H: int, W: int, cfg: dict, mode: str = "fp32") -> dict:
    """algorithmic {kernel: [launches, bytes, flop]} of one engine forward on B images of H x W (fp32: 4 bytes per element)"""
    c = gi.full_cfg(**cfg)
    E, hid, cin, up, head = c["embed_dim"], int(c["embed_dim"] * c["mlp_ratio"]), c["in_chans"], c["upscale"], c["upsampler"]
    ws, _, _ = gi.window_of(cfg)
    w = c["window_size"]
    Hp, Wp = H + (w - H % w) % w, W + (w - W % w) % w
    M = B * Hp * Wp
    out = {k: [0, 0.0, 0.0] for k in KERNELS}
    gk = GEMM_KERNEL[mode]
    out[gk] = out.pop("sw_gemm_kernel")

    def add(k, elems, flop):
        out[k][0] += 1
        out[k][1] += 4.0 * elems
        out[k][2] += float(flop)

    def gemm(rows, K, N, res=False, out_elems=None):
        add(gk, rows * K + K * N + (rows * N if out_elems is None else out_elems) + (rows * N if res else 0), 2 * rows * K * N)

    def resi():
        if c["resi_connection"] == "3conv":
            gemm(M, 9 * E, E // 4)
            gemm(M, E // 4, E // 4)
            gemm(M, 9 * (E // 4), E, res=True)
        else:
            gemm(M, 9 * E, E, res=True)

    add("swinir_pad_kernel", B * cin * (H * W + Hp * Wp), 2 * B * cin * Hp * Wp)
    gemm(M, 9 * cin, E)
    if c["patch_norm"]:
        add("sw_ln_kernel", 2 * M * E, 8 * M * E)
    for depth in c["depths"]:
        for _ in range(depth):
            add("sw_ln_kernel", 2 * M * E, 8 * M * E)
            gemm(M, E, 3 * E)
            add("sw_attn_kernel", 3 * M * E + M * E, 4 * M * ws * ws * E)
            gemm(M, E, E, res=True)
            add("sw_ln_kernel", 2 * M * E, 8 * M * E)
            gemm(M, E, hid)
            gemm(M, hid, E, res=True)
        resi()
    add("sw_ln_kernel", 2 * M * E, 8 * M * E)
    resi()
    Ho, Wo = min(H * up, Hp * (1 if head == "" else up)), min(W * up, Wp * (1 if head == "" else up))
    n_out = B * cin * Ho * Wo
    if head == "pixelshuffle":
        gemm(M, 9 * E, 64)
        r, stages = (3, 1) if up == 3 else (2, int(math.log2(up)))
        rows = M
        for _ in range(stages):
            gemm(rows, 9 * 64, r * r * 64)
            rows *= r * r
        gemm(rows, 9 * 64, cin, out_elems=n_out)
    elif head == "pixelshuffledirect":
        gemm(M, 9 * E, up * up * cin, out_elems=n_out)
    elif head == "nearest+conv":
        gemm(M, 9 * E, 64)
        rows = M
        for _ in range(int(math.log2(up))):
            rows *= 4
            add(gk, rows // 4 * 64 + 9 * 64 * 64 + rows * 64, 2 * rows * 9 * 64 * 64)      # reads the source image, not its 2x copy
        gemm(rows, 9 * 64, 64)
        gemm(rows, 9 * 64, cin, out_elems=n_out)
    else:
        gemm(M, 9 * E, cin, res=True, out_elems=n_out)
    return out


def cmd_counts(a):
    cfg, (H, W) = WORK[a.work]
    per = counts(a.batch, H, W, cfg)
    tot_b, tot_f = sum(v[1] for v in per.values()), sum(v[2] for v in per.values())
    print(json.dumps({"work": a.work, "batch": a.batch, "size": [H, W],
                      "per_kernel": {k: {"launches": v[0], "gbytes": round(v[1] / 1e9, 3), "tflop": round(v[2] / 1e12, 4)} for k, v in per.items()},
                      "total_gbytes": round(tot_b / 1e9, 3), "total_tflop": round(tot_f / 1e12, 4),
                      "ms_at_fp32_peak": round(tot_f / FP32_PEAK * 1e3, 2), "ms_at_bf16x6_nominal": round(tot_f / BF16X6_NOMINAL * 1e3, 2),
                      "ms_at_hbm_peak": round(tot_b / HBM_PEAK * 1e3, 2)}))


def _median_times(fn, iters):
    import torch
    ts = []
    for _ in range(iters):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        ts.append(ev0.elapsed_time(ev1) / 1e3)
    ts.sort()
    n = len(ts)
    return (ts[n // 2] if n % 2 else 0.5 * (ts[n // 2 - 1] + ts[n // 2])), ts[0], ts[-1]


def cmd_time(a):
    import torch
    import swinir_torch as si
    from xmm_superres_denoise.models import SwinIR
    modes = ["fp32", "bf16x6"] if a.math == "both" else [a.math]
    for work in a.work.split(","):
        cfg, (H, W) = WORK[work]
        state = gi.make_state(cfg, 2024)
        m = SwinIR(**gi.full_cfg(**cfg))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        m = m.set_math(modes[0]).cuda()
        sd = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
        tflop = sum(v[2] for v in counts(1, H, W, cfg).values()) / 1e12
        for B in ([1] if work == "dn" else [int(b) for b in a.batches.split(",")]):
            x = torch.from_numpy(gi.make_input((B, 1, H, W), 7)).cuda()
            with torch.no_grad():
                for _ in range(2):          # warm-up: workspace plan, code objects, library algorithm choices
                    m(x)
                    si.swinir_forward(sd, x, **cfg)
                eng = _alternating_times(m, x, modes, a.iters)
                t_eager, lo_t, hi_t = _median_times(lambda: si.swinir_forward(sd, x, **cfg), a.iters)
                y_eager = si.swinir_forward(sd, x, **cfg)
                dmaxs = {k: float((m.set_math(k)(x) - y_eager).abs().max()) for k in modes}
            for k in modes:
                t_eng, lo_e, hi_e = eng[k]
                print(json.dumps({"model": "swinir", "work": work, "math": k, "batch": B, "size": [H, W], "out": list(y_eager.shape[2:]),
                                  "iters": a.iters, "engine_ms": round(t_eng * 1e3, 3),
                                  "engine_ms_min_max": [round(lo_e * 1e3, 3), round(hi_e * 1e3, 3)],
                                  "engine_images_per_s": round(B / t_eng, 2), "torch_eager_fp32_ms": round(t_eager * 1e3, 3),
                                  "torch_eager_fp32_ms_min_max": [round(lo_t * 1e3, 3), round(hi_t * 1e3, 3)],
                                  "engine_over_eager": round(t_eager / t_eng, 3),
                                  "share_of_fp32_matrix_peak": round(B * tflop * 1e12 / t_eng / FP32_PEAK, 4),
                                  "share_of_bf16x6_nominal": round(B * tflop * 1e12 / t_eng / BF16X6_NOMINAL, 4),
                                  "max_abs_diff": dmaxs[k], "device": torch.cuda.get_device_name(0)}), flush=True)
        del m, sd
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--work", default="dn,sr")
    t.add_argument("--batches", default="1,4")
    t.add_argument("--iters", type=int, default=10)
    t.add_argument("--math", default="fp32", choices=["fp32", "bf16x6", "both"])
    c = sub.add_parser("counts")
    c.add_argument("--work", default="dn", choices=sorted(WORK))
    c.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    {"time": cmd_time, "counts": cmd_counts}[a.cmd](a)


if __name__ == "__main__":
    main()
