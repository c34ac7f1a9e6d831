"""`train test` with and without --extended-metrics on one synthetic tree: builds a seeded dataset tree in the
reference layout (411 x 403 counts, 416^2 tiles), fits one epoch for a checkpoint, then runs `test` alternately without and with
the extended collections and reports the wall time of the test epoch alone (train._eval_epoch: every batch composed, run through
the model and the metric collections, ending in the host read of the values), after one warm run of each.

    python tools/ext_metrics_cli_time.py [--n-base 80] [--batch-size 4] [--reps 3]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import dataset_tree as dt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-base", type=int, default=80)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from xmm_superres_denoise import train
    spent = []
    inner = train._eval_epoch

    def timed_epoch(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = {k: float(v) for k, v in inner(*args, **kw).items()}      # the host read ends the epoch
        spent.append(time.perf_counter() - t0)
        return out

    train._eval_epoch = timed_epoch
    with tempfile.TemporaryDirectory() as tmp:
        root = dt.make_sim_tree(os.path.join(tmp, "tree"), n_base=a.n_base, n_agn=4, n_bkg=4, lr_exps=(20,), hr_exp=50, hr_mult=1, seed=1)
        ck = os.path.join(tmp, "ck.pt")
        train.fit("rrdb_denoise", lr_res=416, batch_size=a.batch_size, dataset_dir=root, hr_exp=50, epochs=1, checkpoint=ck, seed=0, log_every=0)
        times = {False: [], True: []}
        for rep in range(a.reps + 1):
            for ext in (False, True):
                spent.clear()
                print(f"--- train test{' --extended-metrics' if ext else ''} (run {rep}{', warm-up' if rep == 0 else ''})", flush=True)
                train.test(ck, root, name="rrdb_denoise", lr_res=416, hr_exp=50, batch_size=a.batch_size, extended_metrics=ext, log=rep == 0)
                print(f"test epoch wall time: {1e3 * spent[-1]:.1f} ms", flush=True)
                if rep:
                    times[ext].append(spent[-1])
        import json
        with open(os.path.join(os.path.dirname(ck), "sim_dataset_sim_img_splits.json")) as f:
            n_test = len(json.load(f).get("test", ()))
        print(f"test split: {n_test} samples, batch {a.batch_size}; median test-epoch wall time over {a.reps} runs: "
              f"without {1e3 * statistics.median(times[False]):.1f} ms, with --extended-metrics {1e3 * statistics.median(times[True]):.1f} ms "
              f"(+{1e3 * (statistics.median(times[True]) - statistics.median(times[False])):.1f} ms)", flush=True)


if __name__ == "__main__":
    main()
