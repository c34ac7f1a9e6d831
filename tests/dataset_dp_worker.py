"""One rank of a data-parallel `fit` fed by the dataset pool (not a test module: started by tests/test_hip_dataset.py, one process
per rank, following tests/dp_worker.py).  Usage:
    RANK=r LOCAL_RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p XSD_DIST_BACKEND=gloo \
        python tests/dataset_dp_worker.py <dataset_dir> <out_dir> <lr_res>
Writes <out_dir>/rank<r>.npz with the flat parameters after the run and the per-step losses."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "xmm-superres-denoise_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch.distributed as dist  # noqa: E402


def run(dataset_dir, out_dir, lr_res):
    from xmm_superres_denoise.train import fit
    rank = int(os.environ["RANK"])
    model, tr, losses = fit("rrdb_denoise", lr_res=lr_res, batch_size=4, dataset_dir=dataset_dir, hr_exp=50, epochs=1, seed=1,
                            splits=os.path.join(out_dir, "splits.json"), log_every=0)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), params=tr.flat.cpu().numpy(), losses=np.array(losses))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2], int(sys.argv[3]))
