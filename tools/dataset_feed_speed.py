"""Dataset feed speed: pool-fed against torch.rand-fed train steps (DESIGN.md "Dataset feed").

Builds a synthetic dataset tree in the reference layout in a temp dir (seeded int32 Poisson counts, 411 x 403 and 822 x 806,
gzip FITS) and times, in one process, at each batch size:
  (a) dataset.batch alone (one xsd_compose_batch launch per resolution);
  (b) DN (rrdb_denoise, HR 50 ks 1x, 416^2) and SR (esr_gen, HR 100 ks 2x, 832^2) train steps fed by the pool;
  (c) the same steps fed by torch.rand tiles of the same shapes, drawn on the host and copied per step as train.fit does
      without a dataset.
Also reports the pool build time and bytes, and the compose kernel's achieved HBM rate against its byte floor.
Prints one JSON line per (batch, model); --out appends them to a file.
    python tools/dataset_feed_speed.py [--batches 1 4 16] [--steps 30] [--out profiles/dataset_feed_speed.jsonl]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import dataset_tree as dt  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-base", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from xmm_superres_denoise.config.config import model_cfg
    from xmm_superres_denoise.data.dataset import XmmDataset
    from xmm_superres_denoise.models import Model
    from xmm_superres_denoise.parallel import DataParallelTrainer
    from xmm_superres_denoise.train import dataset_cfg
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        dt.make_sim_tree(os.path.join(tmp, "dn"), n_base=a.n_base, n_agn=4, n_bkg=4, lr_exps=(20,), hr_exp=50, hr_mult=1, seed=1)
        dt.make_sim_tree(os.path.join(tmp, "sr"), n_base=a.n_base, n_agn=4, n_bkg=4, lr_exps=(20,), hr_exp=100, hr_mult=2, seed=2)
        t_tree = time.perf_counter() - t0
        for kind, name, hr_exp in (("dn", "rrdb_denoise", 50), ("sr", "esr_gen", 100)):
            cfg = dataset_cfg(os.path.join(tmp, kind), name=name, hr_exp=hr_exp)
            t0 = time.perf_counter()
            ds = XmmDataset(cfg).build_pool(device=dev)
            torch.cuda.synchronize()
            t_pool = time.perf_counter() - t0
            hr_res = cfg.hr.res
            for B in a.batches:
                mc = model_cfg(name, batch_size=B)
                model = Model(mc, (416, 416), (hr_res, hr_res))
                model.configure_model()
                model.to(dev)
                tr = DataParallelTrainer(model.model, lr=mc.optimizer.learning_rate, betas=mc.optimizer.betas)
                n = len(ds)
                state = {"i": 0}

                def next_idx():
                    i = state["i"]
                    state["i"] += B
                    return [(i + k) % n for k in range(B)]

                t_batch = timed(lambda: ds.batch(next_idx(), 0), a.steps, a.warmup)
                t_pool_step = timed(lambda: tr.train_step(*ds.batch(next_idx(), 0)), a.steps, a.warmup)
                g = torch.Generator().manual_seed(0)
                t_rand_step = timed(lambda: tr.train_step(torch.rand((B, 1, 416, 416), generator=g).to(dev),
                                                          torch.rand((B, 1, hr_res, hr_res), generator=g).to(dev)), a.steps, a.warmup)
                # byte floor of one batch: the words each sample reads (img + agn [+ bkg]) and the floats it writes
                lr_words, hr_words = ds.lr_pool.shape[0] * ds.lr_pool.shape[1], ds.hr_pool.shape[0] * ds.hr_pool.shape[1]
                floor = B * (4 * (3 * lr_words + 416 * 416) + 4 * (2 * hr_words + hr_res * hr_res))
                line = dict(model=name, batch=B, hr_res=hr_res, batch_ms=t_batch * 1e3, pool_step_ms=t_pool_step * 1e3,
                            rand_step_ms=t_rand_step * 1e3, pool_steps_per_s=1 / t_pool_step, rand_steps_per_s=1 / t_rand_step,
                            pool_vs_rand=t_rand_step / t_pool_step, batch_bytes_floor=floor, batch_tb_per_s=floor / t_batch / 1e12,
                            pool_build_s=t_pool, pool_bytes=ds.pool_bytes, pool_files=len(ds.lr_pool.files) + len(ds.hr_pool.files),
                            tree_write_s=t_tree, steps=a.steps, warmup=a.warmup)
                print(json.dumps(line), flush=True)
                lines.append(line)
                del tr, model
            del ds
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
