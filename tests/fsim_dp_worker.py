"""One rank of a two-rank run of the fsim collection (not a test module: started by tests/test_hip_fsim.py, one process per rank,
following tests/ext_metrics_dp_worker.py).  Usage:
    RANK=r LOCAL_RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/fsim_dp_worker.py <out_dir>
Every rank draws the same four seeded batches and updates the collection with batches r, r + n, ...; after sync() it writes the
epoch values (doubles, before the float32 cast of compute()) to <out_dir>/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def batches(n=4, shape=(2, 64, 80), seed=21):
    import fsim_torch as Fs
    gen = torch.Generator().manual_seed(seed)
    return [tuple(a.float()[:, None] for a in Fs.photon_pair(shape, gen)) for _ in range(n)]


def collection():
    from xmm_superres_denoise.metrics import get_fsim_metrics
    from xmm_superres_denoise.transforms import Normalize
    return get_fsim_metrics(Normalize(1.0, 1.0, "sqrt"), [Normalize(1.0, 1.0, "linear"), Normalize(1.0, 1.0, "sqrt")], "test")


def epoch_values(coll):
    return {f"{mode}/fsim": float(st.compute()) for mode, st in coll.states.items()}


def run(out_dir):
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    coll = collection()
    for p, t in batches()[rank::world]:
        coll.update(p.cuda(), t.cuda())
    coll.sync()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **epoch_values(coll))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1])
