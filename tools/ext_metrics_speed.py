"""Extended test metrics: one xsd_ext_metrics_eval (gmsd, ms_gmsd, haarpsi, msdi, vif_p of a batch) against the plain-torch
restatement of the same formulas (tests/golden/ext_metrics_torch.py) in fp32 ON THE SAME DEVICE, op by op in eager mode
(DESIGN.md section 14).  B = 4 at 416^2 and at 832^2; both sides warm, the repetitions alternate between the two, each
repetition ends in a device synchronise, medians are reported.  One JSON line per size; --out appends them to a file.

    python tools/ext_metrics_speed.py [--reps 30] [--out profiles/ext_metrics_speed.jsonl]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ext_metrics_speed.py --trace     # engine only, 10 evals per size
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import ext_metrics_torch as E  # noqa: E402


def once(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--sizes", type=int, nargs="+", default=[416, 832])
    ap.add_argument("--trace", action="store_true", help="engine only, 10 evals per size after 2 warm ones (for rocprofv3 --kernel-trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from xmm_superres_denoise.engine import ExtMetricsEngine
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    eng = ExtMetricsEngine()
    for S in a.sizes:
        p, t = (v.float().to(dev) for v in E.photon_pair((a.batch, S, S), torch.Generator().manual_seed(S)))

        def engine():
            o = eng.eval(p, t)
            return {"gmsd": o[:, 0], "ms_gmsd": o[:, 1], "haarpsi": o[:, 2], "msdi": o[:, 3], "vif_p": o[:, 4] / o[:, 5]}

        def eager():
            return E.all_metrics(p, t)

        if a.trace:
            for _ in range(12):
                engine()
            torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            once(engine)
            once(eager)
        te, tg = [], []
        for _ in range(a.reps):
            dt_, ve = once(engine)
            te.append(dt_)
            dt_, vg = once(eager)
            tg.append(dt_)
        diff = {n: float(((ve[n] - vg[n].double()).abs() / vg[n].double().abs()).max()) for n in E.NAMES}
        line = {"what": "ext_metrics_eval vs eager torch fp32 restatement, same device, same call", "device": torch.cuda.get_device_name(dev),
                "B": a.batch, "H": S, "W": S, "reps": a.reps, "engine_ms_median": 1e3 * statistics.median(te),
                "engine_ms_min": 1e3 * min(te), "engine_ms_max": 1e3 * max(te), "eager_ms_median": 1e3 * statistics.median(tg),
                "eager_ms_min": 1e3 * min(tg), "eager_ms_max": 1e3 * max(tg),
                "speedup_median": statistics.median(tg) / statistics.median(te), "max_rel_diff_engine_vs_eager": diff}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
