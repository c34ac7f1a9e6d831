"""fsim: one xsd_fsim_eval (piq 0.7.x fsim(chromatic=False) of a batch; parity unpinned) against the plain-torch restatement of the same
formula (tests/golden/fsim_torch.py) in fp32 ON THE SAME DEVICE, op by op in eager mode.  B = 4 at 416^2 and at
832^2; both sides warm, the repetitions alternate between the two, each repetition ends in a device synchronise; medians with min-max
are reported.  The eager side is the restatement as written: like piq it builds the 16 filters and their noise constants on every call;
the engine keeps them in its plan.  One JSON line per size; --out appends them to a file.

    python tools/fsim_speed.py [--reps 20] [--out profiles/r13_fsim_speed.jsonl]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fsim_speed.py --trace     # engine only, 12 evals per size, no counters
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

import fsim_torch as Fs  # noqa: E402


def once(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--sizes", type=int, nargs="+", default=[416, 832])
    ap.add_argument("--trace", action="store_true", help="engine only, 12 evals per size, the warm-up ones among them (for rocprofv3 --kernel-trace; read medians)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from xmm_superres_denoise.engine import FsimEngine
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    eng = FsimEngine()
    for S in a.sizes:
        p, t = (v.float().to(dev) for v in Fs.photon_pair((a.batch, S, S), torch.Generator().manual_seed(S)))

        def engine():
            return eng.eval(p, t)

        def eager():
            return Fs.fsim(p, t)

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
        h, w = Fs.pooled_size(S, S)
        line = {"what": "xsd_fsim_eval vs eager torch fp32 restatement (filters rebuilt per call, as piq does), same device, same process",
                "device": torch.cuda.get_device_name(dev), "B": a.batch, "H": S, "W": S, "pooled": [h, w], "reps": a.reps,
                "engine_ms_median": 1e3 * statistics.median(te), "engine_ms_min": 1e3 * min(te), "engine_ms_max": 1e3 * max(te),
                "eager_ms_median": 1e3 * statistics.median(tg), "eager_ms_min": 1e3 * min(tg), "eager_ms_max": 1e3 * max(tg),
                "eager_over_engine_median": statistics.median(tg) / statistics.median(te),
                "max_rel_diff_engine_vs_eager": float(((ve - vg.double()).abs() / vg.double().abs()).max())}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
