#!/usr/bin/env python3
"""Restormer forward speed on the MI355X: the engine (csrc/restormer.hip) against torch eager fp32 running the float64-oracle's
restatement (tests/golden/restormer_torch.py) in fp32 on the same device, 416 x 416 tiles; --dim 24 (the default: models.toml:58-64, 1 -> 1
channels) or any other width, of which 48 is the published network (3 -> 3 channels, 96 channels per head at decoder level 1: the wide
channel-attention kernels).

  python tools/restormer_speed.py time [--dim 24] [--batches 1,4,16] [--iters 20] [--repeats 1]
                                                                     one JSON line per batch: images/s of both; with --repeats R
                                                                     the median of R timings of --iters forwards, and [min, max]
  python tools/restormer_speed.py hooks [--shape 4,64,1,173056] [--iters 10] [--repeats 5]
                                                                     the channel attention alone through the narrow and the wide
                                                                     test hook (allocation, transpose and sync included in both)
  python tools/restormer_speed.py profile --batch 4 [--iters 5]             engine forwards only (run under rocprofv3 --kernel-trace --stats)
  python tools/restormer_speed.py roof <kernel_stats.csv | results.db> --batch 4 --iters N [--csv-out F]
                                                                     per-kernel time, achieved bytes/s against the HBM roof and
                                                                     FLOP/s against the fp32 peak

The algorithmic bytes / FLOP of each kernel come from the shapes (every operand read once, every result written once), counted by
the code below; kernel times come from rocprofv3's own stats file.  Needs a GPU for `time` and `profile`; `roof` is host arithmetic.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_restormer as gr  # noqa: E402

HBM_PEAK, HBM_MEASURED = 8.0e12, 6.3e12        # MI355X: spec and float4-copy ceiling (bytes/s)
FP32_PEAK = 157.3e12                           # fp32 matrix peak (FLOP/s), the issue's yardstick for the Gram / attention kernels
CFG = dict(inp_channels=1, out_channels=1, dim=24)


def cfg_of(dim: int) -> dict:
    """the XMM configuration at `dim` (1 -> 1 channels); dim 48 is Restormer() as published, 3 -> 3 channels"""
    return {} if dim == 48 else dict(CFG, dim=dim)


def counts(B: int, H: int, W: int, cfg=CFG) -> dict:
    """algorithmic {kernel: [launches, bytes, flop]} of one engine forward"""
    c = gr.full_cfg(**cfg)
    d, f, heads, nb = c["dim"], c["ffn_expansion_factor"], c["heads"], c["num_blocks"]
    out = {k: [0, 0.0, 0.0] for k in ("rst_pw_kernel", "rst_dw_kernel", "rst_gram_kernel", "rst_attn_kernel", "rst_wgram_kernel",
                                      "rst_wsoftmax_kernel", "rst_wfold_kernel", "rst_conv3_kernel")}

    def add(k, nbytes, flop):
        out[k][0] += 1
        out[k][1] += 4.0 * nbytes
        out[k][2] += flop

    def block(C, h, HW):
        hid, ch, n = int(C * f), C // h, B * HW
        add("rst_pw_kernel", (C + 3 * C) * n, 2.0 * C * 3 * C * n)                  # LayerNorm + qkv
        add("rst_dw_kernel", 6 * C * n, 18.0 * 3 * C * n)                            # qkv_dwconv
        part = 2 * B * h * (ch * ch + 2 * ch) * -(-HW // 1024)                       # the double partials, in floats
        if ch <= 64:
            add("rst_gram_kernel", 2 * C * n, 2.0 * (C * ch + 2 * C) * n)            # q k^T and the row norms
            add("rst_attn_kernel", part + B * C * C, B * (2.0 * C * C * ch))         # double partials in
        else:
            # the Gram in 64 x 64 tiles: every tile row reads its q rows once per tile column and the other way round, so q and k are
            # read ceil(ch / 64) times; the FLOP are those of the entries inside the head (rows past it are skipped in groups of 16)
            nt = -(-ch // 64)
            add("rst_wgram_kernel", nt * 2 * C * n + part, 2.0 * (C * ch + 2 * C) * n)
            add("rst_wsoftmax_kernel", part + B * C * ch, B * 10.0 * C * ch)
            add("rst_wfold_kernel", B * (C * ch + 2 * C * C), B * (2.0 * C * C * ch))
        add("rst_pw_kernel", 3 * C * n, 2.0 * C * C * n)                             # (W_po attn) v + residual
        add("rst_pw_kernel", (C + 2 * hid) * n, 2.0 * C * 2 * hid * n)               # LayerNorm + project_in
        add("rst_dw_kernel", 3 * hid * n, (36.0 * hid + 10.0 * hid) * n)             # dwconv + gelu gate
        add("rst_pw_kernel", (hid + 2 * C) * n, 2.0 * hid * C * n)                   # project_out + residual

    def conv3(cin, cout, HW):
        add("rst_conv3_kernel", (cin + cout) * B * HW, 18.0 * cin * cout * B * HW)

    HW1 = H * W
    conv3(c["inp_channels"], d, HW1)
    for _ in range(nb[0]): block(d, heads[0], HW1)
    conv3(d, d // 2, HW1)
    for _ in range(nb[1]): block(2 * d, heads[1], HW1 // 4)
    conv3(2 * d, d, HW1 // 4)
    for _ in range(nb[2]): block(4 * d, heads[2], HW1 // 16)
    conv3(4 * d, 2 * d, HW1 // 16)
    for _ in range(nb[3]): block(8 * d, heads[3], HW1 // 64)
    conv3(8 * d, 16 * d, HW1 // 64)
    add("rst_pw_kernel", (8 * d + 4 * d) * B * HW1 // 16, 2.0 * 8 * d * 4 * d * B * HW1 // 16)
    for _ in range(nb[2]): block(4 * d, heads[2], HW1 // 16)
    conv3(4 * d, 8 * d, HW1 // 16)
    add("rst_pw_kernel", (4 * d + 2 * d) * B * HW1 // 4, 2.0 * 4 * d * 2 * d * B * HW1 // 4)
    for _ in range(nb[1]): block(2 * d, heads[1], HW1 // 4)
    conv3(2 * d, 4 * d, HW1 // 4)
    for _ in range(nb[0] + c["num_refinement_blocks"]): block(2 * d, heads[0], HW1)
    conv3(2 * d, c["out_channels"], HW1)
    return out


def _stat(ts):
    ts = sorted(ts)
    n = len(ts)
    return (ts[n // 2] if n % 2 else 0.5 * (ts[n // 2 - 1] + ts[n // 2])), ts[0], ts[-1]


def _time(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / 1e3 / iters


def cmd_time(a):
    import torch
    import restormer_torch as rt
    from xmm_superres_denoise.models import Restormer
    cfg = cfg_of(a.dim)
    full = gr.full_cfg(**cfg)
    state = gr.make_state(cfg, 2024)
    m = Restormer(**full)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    m = m.cuda()
    sd = {k: torch.from_numpy(v).cuda() for k, v in state.items()}
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.from_numpy(gr.make_input((B, full["inp_channels"], a.size, a.size), 7)).cuda()
        with torch.no_grad():
            for _ in range(2):          # warm-up: workspace plan, code objects, library algorithm choices
                m(x)
                rt.restormer_forward(sd, x, **full)
            t_engs = [_time(lambda: m(x), a.iters) for _ in range(a.repeats)]
            t_eagers = [_time(lambda: rt.restormer_forward(sd, x, **full), a.iters) for _ in range(a.repeats)]
            dmax = float((m(x) - rt.restormer_forward(sd, x, **full)).abs().max())
        (t_eng, e_lo, e_hi), (t_eager, g_lo, g_hi) = _stat(t_engs), _stat(t_eagers)
        line = {"batch": B, "size": a.size, "iters": a.iters, "engine_ms": round(t_eng * 1e3, 3),
                "engine_images_per_s": round(B / t_eng, 2), "torch_eager_fp32_ms": round(t_eager * 1e3, 3),
                "torch_eager_fp32_images_per_s": round(B / t_eager, 2), "engine_over_eager": round(t_eager / t_eng, 3),
                "max_abs_diff": dmax, "device": torch.cuda.get_device_name(0)}
        if a.dim != 24 or a.repeats != 1:
            line.update({"dim": a.dim, "repeats": a.repeats, "engine_ms_min_max": [round(e_lo * 1e3, 3), round(e_hi * 1e3, 3)],
                         "torch_eager_fp32_ms_min_max": [round(g_lo * 1e3, 3), round(g_hi * 1e3, 3)]})
        print(json.dumps(line), flush=True)


def cmd_hooks(a):
    """the channel attention alone at one shape both paths take (at most 64 channels per head), through the two test hooks"""
    import torch
    from xmm_superres_denoise.engine import restormer_channel_attention, restormer_channel_attention_wide
    B, C, heads, HW = (int(v) for v in a.shape.split(","))
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, 3 * C, HW, generator=g).cuda()
    temp = (torch.rand(heads, generator=g) + 0.5).cuda()
    wpo = ((torch.rand(C, C, generator=g) * 2 - 1) / C ** 0.5).cuda()
    x0 = torch.randn(B, C, HW, generator=g).cuda()
    out, ts = {}, {}
    for name, fn in (("narrow", restormer_channel_attention), ("wide", restormer_channel_attention_wide)):
        x = x0.clone()
        out[name] = fn(qkv, temp, wpo, None, x0.clone(), heads)
        ts[name] = _stat([_time(lambda: fn(qkv, temp, wpo, None, x, heads), a.iters) for _ in range(a.repeats)])
    print(json.dumps({"hooks": [B, C, heads, HW], "iters": a.iters, "repeats": a.repeats,
                      "narrow_ms": round(ts["narrow"][0] * 1e3, 3), "narrow_ms_min_max": [round(v * 1e3, 3) for v in ts["narrow"][1:]],
                      "wide_ms": round(ts["wide"][0] * 1e3, 3), "wide_ms_min_max": [round(v * 1e3, 3) for v in ts["wide"][1:]],
                      "wide_over_narrow": round(ts["wide"][0] / ts["narrow"][0], 3), "bitwise_equal": bool(torch.equal(out["narrow"], out["wide"])),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def cmd_profile(a):
    import torch
    from xmm_superres_denoise.models import Restormer
    full = gr.full_cfg(**cfg_of(a.dim))
    m = Restormer(**full).cuda()
    x = torch.from_numpy(gr.make_input((a.batch, full["inp_channels"], a.size, a.size), 7)).cuda()
    with torch.no_grad():
        m(x)            # first forward: plan + pack (the stats file counts it: `roof` takes iters + 1 forwards)
        for _ in range(a.iters):
            m(x)
    torch.cuda.synchronize()
    print(json.dumps({"profiled_forwards": a.iters + 1, "batch": a.batch, "size": a.size}))


def stats_rows(path):
    """kernel stats rows {Name, Calls, TotalDurationNs} from rocprofv3's kernel_stats.csv or from its results database (the
    `top_kernels` view of the .db that rocprofv3 writes by default; durations there are in microseconds)"""
    if not path.endswith(".db"):
        return list(csv.DictReader(open(path)))
    import sqlite3
    db = sqlite3.connect(path)
    return [{"Name": n, "Calls": c, "TotalDurationNs": t * 1e3, "AverageNs": avg * 1e3, "Percentage": pct}
            for n, c, t, avg, pct in db.execute("select name, total_calls, total_duration, average, percentage from top_kernels")]


def cmd_roof(a):
    per = counts(a.batch, a.size, a.size, cfg_of(a.dim))
    n_fwd = a.iters + 1
    rows = stats_rows(a.stats)
    if a.csv_out:
        with open(a.csv_out, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage"], extrasaction="ignore")
            w.writeheader()
            w.writerows(rows)
    print(f"# kernel, calls, total ms, ms per forward, GB/s achieved, share of 8.0 TB/s (of 6.3 measured), GFLOP/s, share of 157 TF/s; "
          f"B = {a.batch}, {a.size} x {a.size}, {n_fwd} forwards")
    for r in rows:
        name = r.get("Name", r.get("KernelName", ""))
        key = next((k for k in per if k in name), None)
        if key is None:
            continue
        tot_s = float(r["TotalDurationNs"]) * 1e-9
        launches, nbytes, flop = per[key]
        bps, fps = nbytes * n_fwd / tot_s, flop * n_fwd / tot_s
        print(f"{key}, {r['Calls']} (expected {launches * n_fwd}), {tot_s * 1e3:.3f}, {tot_s * 1e3 / n_fwd:.3f}, {bps / 1e9:.0f}, "
              f"{bps / HBM_PEAK:.3f} ({bps / HBM_MEASURED:.3f}), {fps / 1e9:.0f}, {fps / FP32_PEAK:.4f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--batches", default="1,4,16")
    t.add_argument("--iters", type=int, default=10)
    t.add_argument("--size", type=int, default=416)
    t.add_argument("--repeats", type=int, default=1, help="timings of --iters forwards each: the median and [min, max] are reported")
    h = sub.add_parser("hooks")
    h.add_argument("--shape", default="4,64,1,173056", help="B,C,heads,HW with at most 64 channels per head")
    h.add_argument("--iters", type=int, default=10)
    h.add_argument("--repeats", type=int, default=5)
    p = sub.add_parser("profile")
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--size", type=int, default=416)
    r = sub.add_parser("roof")
    r.add_argument("stats")
    r.add_argument("--batch", type=int, default=4)
    r.add_argument("--iters", type=int, default=5)
    r.add_argument("--size", type=int, default=416)
    r.add_argument("--csv-out", default=None, help="also write the kernel stats as CSV")
    for q in (t, p, r):
        q.add_argument("--dim", type=int, default=24, help="24: the XMM configuration; 48: Restormer() as published (3 -> 3 channels)")
    a = ap.parse_args()
    {"time": cmd_time, "hooks": cmd_hooks, "profile": cmd_profile, "roof": cmd_roof}[a.cmd](a)


if __name__ == "__main__":
    main()
