"""Training driver: the engine-side counterpart of the reference's `train.py fit` (train.py:19-171) for the two RRDB
models, without Lightning.  One process per GPU (launch with torch.distributed.run for N > 1); data parallelism and the
optimizer are `parallel.DataParallelTrainer` (flat-buffer RCCL all-reduce overlapped with backward + fused Adam).

Without a dataset the feed is the reference's `BoringDataset` analogue (random tensors of the configured shapes,
data/dataset.py:52-74).  With `dataset_dir` it is the reference's XmmDataset (data/dataset.py): every file is inflated once
into a device pool of raw FITS words, and each batch is one `xsd_compose_batch` launch per resolution (img + agn +
background, mask, upsample, pad, normalize); `fit` then validates every epoch, keeps the best val/loss checkpoint and tests it,
and `test` evaluates a checkpoint on the test split.  `extended_metrics=True` (CLI --extended-metrics) adds the reference's
get_ext_metrics / get_in_ext_metrics to the test epoch (vif_p, gmsd, ms_gmsd, haarpsi, msdi; without fsim).  `fsim=True` (CLI --fsim),
independent of it, adds the sixth metric as key families of its own, test/<mode>/fsim and test/<mode>/in/fsim (csrc/fsim.hip; parity
unpinned): opt-in, because the extended collection's refusal of fsim and its notice text are pinned by tests.

Checkpoints use the reference's Lightning layout: {"state_dict": {"model.<key>": tensor}} with the reference key names,
so `Model.load_from_checkpoint`-style consumers (utils/run_inference_on_file.py:28-35) can read them.
"""
from __future__ import annotations

import argparse
import os

import torch
import torch.distributed as dist

from xmm_superres_denoise.config.config import model_cfg
from xmm_superres_denoise.models import Model
from xmm_superres_denoise.parallel import DataParallelTrainer


def save_checkpoint(path: str, model: Model, trainer: DataParallelTrainer, epoch: int) -> None:
    sd = {"model." + k: v.detach().cpu() for k, v in model.model.state_dict().items()}
    torch.save({"state_dict": sd, "epoch": epoch, "global_step": trainer.step_count,
                "adam": {"m": trainer.m.cpu(), "v": trainer.v.cpu(), "step": trainer.step_count}}, path)


def load_checkpoint(path: str, model: Model, trainer: DataParallelTrainer | None = None) -> dict:
    """Reads a checkpoint with the loader that executes nothing from the file (`weights_only=True`: tensors, numbers, strings,
    dicts / lists of them).  What save_checkpoint writes is exactly that; a Lightning `.ckpt` carrying pickled objects
    (callback states, hyper-parameter namespaces) is refused rather than unpickled: the error raised here names what is accepted
    and the one-liner that reduces such a file to {"state_dict": ...} on a machine the user trusts."""
    import pickle
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:      # a Lightning .ckpt with objects under hyper_parameters / callbacks
        raise RuntimeError(
            f"{path}: the safe loader (weights_only=True) refused this checkpoint -- it holds pickled objects besides tensors and plain "
            "containers (a genuine Lightning .ckpt carries them under `hyper_parameters` / `callbacks`).  Accepted: a file whose "
            "`state_dict` maps the reference's key names (with or without Lightning's `model.` prefix) to tensors, optionally with this "
            "driver's `adam` block.  Reduce it on a machine you trust: torch.save({'state_dict': torch.load(path, weights_only=False)"
            f"['state_dict']}}, out).  ({e})") from e
    if not isinstance(ck, dict) or "state_dict" not in ck:
        raise RuntimeError(f"{path}: no `state_dict` in this checkpoint (keys: {sorted(ck) if isinstance(ck, dict) else type(ck).__name__})")
    raw = ck["state_dict"]
    # Lightning prefixes the generator's keys with the attribute name (`model.`, models/model.py:157-186); a bare state_dict is taken as is
    sd = {k[len("model."):]: v for k, v in raw.items() if k.startswith("model.")} or dict(raw)
    if model.model is None:
        model.configure_model()
    model.model.load_state_dict(sd)
    if trainer is not None and "adam" in ck:
        trainer.m.copy_(ck["adam"]["m"]); trainer.v.copy_(ck["adam"]["v"]); trainer.step_count = int(ck["adam"]["step"])
    return ck


def fit(name: str = "rrdb_denoise", lr_res: int = 416, batch_size: int = 4, steps: int = 10, device: str | None = None,
        checkpoint: str | None = None, seed: int = 0, math: str | None = None, log_every: int = 1,
        loss: str = "l1", scaling: str = "linear", val_batches: int = 0, dataset_dir: str | None = None,
        dataset_name: str = "sim_dataset", dataset_type: str = "sim", lr_exps=(20,), hr_exp: int = 100, epochs: int = 1,
        lr_det_mask: str | None = None, hr_det_mask: str | None = None, agn: int = 1, lr_bkg: int = 1, comb_hr: bool = False,
        splits: str | None = None, max_pool_bytes: int | None = None, extended_metrics: bool = False, fsim: bool = False):
    """loss: "l1" (BASELINE configs[2]) or "paper" = the reference's shipped default, 0.5 psnr + 0.5 ms_ssim with the
    scaling table of the dataset's stretch mode (`scaling`; res/configs/loss_functions.toml, train.py:46-63).

    Without `dataset_dir`: random tiles for `steps` steps (the reference's BoringDataset analogue).  With it: the reference's
    `fit` on an XMM FITS tree (`<dataset_dir>/<dataset_name>/{img,agn,bkg}/<exp>ks/**/<mult>x/`, or real data): `epochs`
    epochs of shuffled train shards, each followed by a validation epoch (loss + get_metrics + get_in_metrics over the
    `linear` normaliser, train.py:72-88); the checkpoint of the lowest val/loss is kept (ModelCheckpoint(monitor="val/loss",
    mode="min")), then a test epoch runs on it.  `scaling` is then the dataset's stretch; lr_res is the dataset's lr.res.
    The split JSON goes to `splits` (default: next to the checkpoint).  `extended_metrics` adds get_ext_metrics / get_in_ext_metrics
    to that final test epoch only (the reference builds them only for `test`, train.py:90-102); `fsim` adds get_fsim_metrics /
    get_in_fsim_metrics to the same epoch, with or without `extended_metrics`."""
    if name == "restormer":
        raise NotImplementedError("restormer: training Restormer is not on the MI355X engine (forward only: inference, infer.py, "
                                  "validation / test metrics); fit supports rrdb_denoise and esr_gen")
    if name == "swinfir":
        raise NotImplementedError("swinfir: training SwinFIR is not on the MI355X engine (forward only: inference, infer.py, "
                                  "validation / test metrics); fit supports rrdb_denoise and esr_gen")
    if name == "hat":
        raise NotImplementedError("hat: training HAT is not on the MI355X engine (forward only: inference, infer.py, "
                                  "validation / test metrics); fit supports rrdb_denoise and esr_gen")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # one process per GPU over RCCL ("nccl"); XSD_DIST_BACKEND=gloo rehearses N ranks on fewer GPUs (ranks then share devices),
    # exactly as bench.py does
    backend = os.environ.get("XSD_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if ndev < 1:
        raise RuntimeError("train.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    if backend == "nccl" and world > ndev:
        raise RuntimeError(f"{world} ranks but {ndev} GPU(s): RCCL needs one GPU per rank (XSD_DIST_BACKEND=gloo rehearses the "
                           "multi-rank path on fewer GPUs)")
    dev = torch.device(device or f"cuda:{local_rank if backend == 'nccl' else local_rank % ndev}")
    torch.cuda.set_device(dev)
    force_dp = os.environ.get("XSD_FORCE_DP", "0") == "1"      # one rank, collectives on: the RCCL path on a single GPU (parallel.collectives_on)
    if (world > 1 or force_dp) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if dataset_dir is not None:
        return _fit_dataset(name, batch_size, dev, rank, world, checkpoint, seed, math, log_every, loss, scaling,
                            dataset_cfg(dataset_dir, dataset_name, dataset_type, name, lr_res, lr_exps, hr_exp, lr_det_mask,
                                        hr_det_mask, agn, lr_bkg, comb_hr, scaling, batch_size),
                            epochs, splits, max_pool_bytes, extended_metrics, fsim)
    cfg = model_cfg(name, batch_size=batch_size)
    hr_res = lr_res * (2 if name == "esr_gen" else 1)
    torch.manual_seed(seed)
    from xmm_superres_denoise.utils import Loss, create_loss, load_loss_config
    loss_fn = None
    if loss != "l1":
        loss_fn = create_loss(*load_loss_config(scaling))
    metrics = None
    if val_batches > 0:   # train.py:86-104 of the reference: metric collections over the scaling normalizers
        from xmm_superres_denoise.metrics import get_metrics
        from xmm_superres_denoise.transforms import Normalize
        norm = Normalize(lr_max=0.0022336, hr_max=0.0022336 if name == "rrdb_denoise" else 0.0005584, stretch_mode=scaling)
        metrics = get_metrics(norm, [Normalize(norm.lr_max.item(), norm.hr_max.item(), "linear")], "val")
    model = Model(cfg, (lr_res, lr_res), (hr_res, hr_res), loss=loss_fn if loss_fn is not None else Loss({"l1": 1.0}),
                  metrics=metrics, extended_metrics=None,
                  in_metrics=None, in_extended_metrics=None)
    model.configure_model()
    model.to(dev)
    if math:
        model.model.set_math(math)
    trainer = DataParallelTrainer(model.model, lr=cfg.optimizer.learning_rate, betas=cfg.optimizer.betas, loss=loss_fn)
    per_rank = batch_size // world if batch_size % world == 0 else batch_size
    g = torch.Generator().manual_seed(seed + 1 + rank)
    losses = []
    for it in range(steps):
        lr_img = torch.rand((per_rank, 1, lr_res, lr_res), generator=g).to(dev)   # BoringDataset analogue
        hr_img = torch.rand((per_rank, 1, hr_res, hr_res), generator=g).to(dev)
        loss = trainer.global_loss(trainer.train_step(lr_img, hr_img))
        losses.append(float(loss))
        if rank == 0 and log_every and it % log_every == 0:
            print(f"step {it}: train/loss {losses[-1]:.6f}", flush=True)
    if val_batches > 0:       # one validation epoch (reference model.py:53-60); metric states are reduced over the ranks
        model.on_validation_start()                                    # inside on_validation_epoch_end (sum / min / max)
        for _ in range(val_batches):
            lr_img = torch.rand((per_rank, 1, lr_res, lr_res), generator=g).to(dev)
            hr_img = torch.rand((per_rank, 1, hr_res, hr_res), generator=g).to(dev)
            model.validation_step((lr_img, hr_img))
        logged = model.on_validation_epoch_end()
        if rank == 0 and log_every:
            print("validation: " + ", ".join(f"{k} {float(v):.6f}" for k, v in sorted(logged.items())), flush=True)
    if checkpoint and rank == 0:
        save_checkpoint(checkpoint, model, trainer, epoch=0)
    return model, trainer, losses


class SwinIRTrainer:
    """What fit_swinir and fit_swinfir train with (the net: a TrainableSwinIR or a TrainableSwinFIR), in the shape save_checkpoint /
    load_checkpoint expect of a trainer (`m`, `v`, `step_count`) and of a
    model (`model`: the wrapped SwinIR, whose state dict has the reference's key names).  The optimizer is torch.optim.Adam over the
    SwinIR's own Parameter objects with the reference's rule (lr, betas, eps 1e-8, no weight decay); its moments are views into the
    two flat buffers `m` and `v` (parameter order), which is what the `adam` block of a checkpoint holds.

    Why torch.optim.Adam and not the engine's xsd_adam_step: that entry belongs to an RRDB engine handle and steps ONE flat buffer
    with its flat gradient; here autograd delivers one gradient tensor per parameter and the parameters move into a flat buffer only
    when the fused forward first runs, so the flat form would cost a gather per step for an elementwise update that is a fraction of a
    percent of the step."""

    def __init__(self, net, lr: float = 2e-4, betas=(0.9, 0.999), loss=None):
        self.net, self.model, self.loss = net, net.module, loss
        self.params = [p for p in self.model.parameters() if p.requires_grad]
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.opt = torch.optim.Adam(self.params, lr=lr, betas=tuple(betas), eps=1e-8, weight_decay=0.0)
        off = 0
        for p in self.params:
            k = p.numel()
            self.opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": self.m[off:off + k].view(p.shape),
                                 "exp_avg_sq": self.v[off:off + k].view(p.shape)}
            off += k

    @property
    def step_count(self) -> int:
        return int(self.opt.state[self.params[0]]["step"].item())

    @step_count.setter
    def step_count(self, n: int):
        for p in self.params:
            self.opt.state[p]["step"].fill_(float(n))

    def train_step(self, lr_img: torch.Tensor, hr_img: torch.Tensor) -> torch.Tensor:
        self.net.train()
        self.opt.zero_grad(set_to_none=True)
        y = self.net(lr_img)
        if self.loss is None:
            loss = torch.nn.functional.l1_loss(y, hr_img)
            loss.backward()
        else:       # the composed loss is an engine kernel with its own gradient (utils.Loss.value_and_grad)
            loss, dy = self.loss.value_and_grad(y.detach().contiguous(), hr_img)
            y.backward(dy)
        self.opt.step()
        return loss.detach()


def fit_swinir(ctor_kwargs: dict, steps: int = 10, batch_size: int = 1, lr_res: int = 64, data=None, lr: float = 2e-4,
               betas=(0.9, 0.999), loss="l1", clamp: bool = False, seed: int = 0, checkpoint: str | None = None,
               device: str | None = None, log_every: int = 1):
    """Train a SwinIR on the MI355X engine: `SwinIR(**ctor_kwargs)` (the reference's constructor arguments), wrapped in a
    TrainableSwinIR (models/modules/swinir_train.py: the forward composed of the differentiable HIP ops of xmm_superres_denoise/ops.py),
    Adam with the reference's rule.  Single device; `fit` is untouched and keeps refusing the transformers by name.

    data: None = random tiles for `steps` steps (the BoringDataset analogue of `fit`: lr [B, in_chans, lr_res, lr_res], or
    [B, in_chans, H, W] where lr_res is a pair (H, W); hr at the network's output size), or any iterable of (lr, hr) CUDA batches, e.g.
    `(dm.dataset.batch(idx, 0) for idx in dm.batches("train", batch_size, 0))` of an XmmDataModule (at most `steps` of them; steps=None
    takes them all).  loss: "l1" (torch's l1_loss on the output: one elementwise pass; the engine's xsd_l1_loss belongs to an RRDB engine
    handle) or a create_loss(...) object (the engine's loss kernels with their own gradient).  clamp: the [0, 1] clamp of Model.forward on the training output.
    checkpoint: written in save_checkpoint's layout (reference key names + the `adam` block); infer.load_swinir(checkpoint,
    **ctor_kwargs) loads it and load_checkpoint(path, trainer, trainer) restores the moments.
    Returns (trainable net, trainer, losses)."""
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    return _fit_wrapped("fit_swinir", SwinIR, TrainableSwinIR, lambda m, h, w: m.out_size(h, w), ctor_kwargs, steps, batch_size, lr_res,
                        data, lr, betas, loss, clamp, seed, checkpoint, device, log_every)


def fit_swinfir(ctor_kwargs: dict, steps: int = 10, batch_size: int = 1, lr_res: int = 64, data=None, lr: float = 2e-4,
                betas=(0.9, 0.999), loss="l1", clamp: bool = False, seed: int = 0, checkpoint: str | None = None,
                device: str | None = None, log_every: int = 1):
    """Train a SwinFIR on the MI355X engine: `SwinFIR(**ctor_kwargs)` (the reference's constructor arguments, with
    resi_connection="1conv": "SFB" is refused by name), wrapped in a TrainableSwinFIR (models/modules/swinfir_train.py: the forward
    composed of the differentiable HIP ops of xmm_superres_denoise/ops.py).  Everything else is fit_swinir's: the data, the loss, the
    clamp, Adam with its moments in two flat buffers, the checkpoint layout (SwinFIR(**ctor_kwargs) loads its `state_dict` minus the
    `model.` prefix; load_checkpoint(path, trainer, trainer) restores the moments).  lr_res (one side, or (H, W)) must lie on the
    window grid.  `fit` is untouched and keeps refusing "swinfir" by name.  Returns (trainable net, trainer, losses)."""
    from xmm_superres_denoise.models import SwinFIR, TrainableSwinFIR
    return _fit_wrapped("fit_swinfir", SwinFIR, TrainableSwinFIR, lambda m, h, w: (h * m.upscale, w * m.upscale), ctor_kwargs, steps,
                        batch_size, lr_res, data, lr, betas, loss, clamp, seed, checkpoint, device, log_every)


def fit_hat(ctor_kwargs: dict, steps: int = 10, batch_size: int = 1, lr_res: int = 64, data=None, lr: float = 2e-4,
            betas=(0.9, 0.999), loss="l1", clamp: bool = False, seed: int = 0, checkpoint: str | None = None,
            device: str | None = None, log_every: int = 1):
    """Train a HAT on the MI355X engine: `HAT(**ctor_kwargs)` (the reference's constructor arguments; upsampler "pixelshuffle",
    resi_connection "1conv" or "identity"), wrapped in a TrainableHAT (models/modules/hat_train.py: the forward composed of the
    differentiable HIP ops of xmm_superres_denoise/ops.py, with overlap_attention and channel_attention for the OCAB and the CAB).
    Everything else is fit_swinir's: the data, the loss, the clamp, Adam with its moments in two flat buffers, the checkpoint layout
    (the reference's key names with the `model.` prefix: infer.load_model(path, "hat") loads a checkpoint of the models.toml
    configuration, HAT(**ctor_kwargs) loads its `state_dict` minus the prefix; load_checkpoint(path, trainer, trainer) restores the
    moments).  The default lr is the reference's for [hat] (models.toml: learning_rate = 0.0002).  lr_res (one side, or (H, W)) must lie
    on the window grid.  `fit` is untouched and keeps refusing "hat" by name.  Returns (trainable net, trainer, losses)."""
    from xmm_superres_denoise.models import HAT, TrainableHAT
    return _fit_wrapped("fit_hat", HAT, TrainableHAT, lambda m, h, w: (h * m.upscale, w * m.upscale), ctor_kwargs, steps, batch_size,
                        lr_res, data, lr, betas, loss, clamp, seed, checkpoint, device, log_every)


def _fit_wrapped(what, module_cls, wrapper_cls, out_size, ctor_kwargs, steps, batch_size, lr_res, data, lr, betas, loss, clamp, seed,
                 checkpoint, device, log_every):
    """the one body of fit_swinir, fit_swinfir and fit_hat: a forward-only module of models/, its trainable wrapper, SwinIRTrainer"""
    if torch.cuda.device_count() < 1:
        raise RuntimeError("train.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    if loss != "l1" and not hasattr(loss, "value_and_grad"):
        raise ValueError(f"{what}: loss {loss!r} is not supported (\"l1\" or a create_loss(...) object)")
    dev = torch.device(device or "cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(seed)
    module = module_cls(**ctor_kwargs).to(dev)
    net = wrapper_cls(module, generator=torch.Generator(device=dev).manual_seed(seed + 2), clamp=clamp)
    trainer = SwinIRTrainer(net, lr=lr, betas=betas, loss=None if loss == "l1" else loss)
    if data is None:
        g = torch.Generator().manual_seed(seed + 1)
        rh, rw = (lr_res, lr_res) if isinstance(lr_res, int) else (int(v) for v in lr_res)      # a square tile, or (H, W)
        Ho, Wo = out_size(module, rh, rw)

        def tiles():
            while True:
                yield (torch.rand((batch_size, module.in_chans, rh, rw), generator=g).to(dev),
                       torch.rand((batch_size, module.in_chans, Ho, Wo), generator=g).to(dev))
        data = tiles()
        steps = 10 if steps is None else steps
    losses = []
    for it, (lr_img, hr_img) in enumerate(data):
        if steps is not None and it >= steps:
            break
        losses.append(float(trainer.train_step(lr_img, hr_img)))
        if log_every and it % log_every == 0:
            print(f"step {it}: train/loss {losses[-1]:.6f}", flush=True)
    net.eval()
    if checkpoint:
        save_checkpoint(checkpoint, trainer, trainer, epoch=0)
    return net, trainer, losses


def dataset_cfg(dataset_dir, dataset_name="sim_dataset", dataset_type="sim", name="rrdb_denoise", lr_res=416, lr_exps=(20,),
                hr_exp=100, lr_det_mask=None, hr_det_mask=None, agn=1, lr_bkg=1, comb_hr=False, scaling="sqrt", batch_size=1):
    """the [dataset] section of the reference's run config (res/baseline_config.toml) for `name`: HR at lr_res for the
    denoiser, 2 x lr_res for esr_gen / swinfir / hat; clamp_max values of the baseline config"""
    from xmm_superres_denoise.config.config import DatasetCfg, HrDatasetCfg, LrDatasetCfg
    hr_res = lr_res * (2 if name in ("esr_gen", "swinfir", "hat") else 1)
    return DatasetCfg(directory=dataset_dir, name=dataset_name, type=dataset_type, agn=agn, comb_hr=comb_hr, scaling=scaling,
                      batch_size=batch_size,
                      lr=LrDatasetCfg(bkg=lr_bkg, det_mask=lr_det_mask, exps=list(lr_exps), res=lr_res),
                      hr=HrDatasetCfg(det_mask=hr_det_mask, exp=hr_exp, res=hr_res))


def _metric_sets(dcfg, stage: str):
    """get_metrics / get_in_metrics of the reference's train.py:68-88: the dataset normaliser and the `linear` scaling one"""
    from xmm_superres_denoise.metrics import get_in_metrics, get_metrics
    from xmm_superres_denoise.transforms import Normalize
    norm = Normalize(lr_max=dcfg.lr.clamp_max, hr_max=dcfg.hr.clamp_max, stretch_mode=dcfg.scaling)
    lin = [Normalize(lr_max=dcfg.lr.clamp_max, hr_max=dcfg.hr.clamp_max, stretch_mode="linear")]
    return get_metrics(norm, lin, stage), get_in_metrics(norm, lin, stage)


def _ext_metric_sets(dcfg, stage: str):
    """get_ext_metrics / get_in_ext_metrics of the reference's train.py:90-102 (built for `test` only), same normalisers"""
    from xmm_superres_denoise.metrics import get_ext_metrics, get_in_ext_metrics
    from xmm_superres_denoise.transforms import Normalize
    norm = Normalize(lr_max=dcfg.lr.clamp_max, hr_max=dcfg.hr.clamp_max, stretch_mode=dcfg.scaling)
    lin = [Normalize(lr_max=dcfg.lr.clamp_max, hr_max=dcfg.hr.clamp_max, stretch_mode="linear")]
    return get_ext_metrics(norm, lin, stage), get_in_ext_metrics(norm, lin, stage)


def _fsim_metric_sets(dcfg, stage: str):
    """get_fsim_metrics / get_in_fsim_metrics (the `fsim` entry of the reference's extended set), same normalisers"""
    from xmm_superres_denoise.metrics import get_fsim_metrics, get_in_fsim_metrics
    from xmm_superres_denoise.transforms import Normalize
    norm = Normalize(lr_max=dcfg.lr.clamp_max, hr_max=dcfg.hr.clamp_max, stretch_mode=dcfg.scaling)
    lin = [Normalize(lr_max=dcfg.lr.clamp_max, hr_max=dcfg.hr.clamp_max, stretch_mode="linear")]
    return get_fsim_metrics(norm, lin, stage), get_in_fsim_metrics(norm, lin, stage)


EXT_METRICS_NOTICE = ("test: the extended metric collection (get_ext_metrics / get_in_ext_metrics: piq and VIF) is not on the "
                      "MI355X engine and is not computed; reported: loss, get_metrics and get_in_metrics")
EXT_METRICS_ON_NOTICE = ("test: extended metrics (get_ext_metrics / get_in_ext_metrics) computed on the MI355X engine: vif_p, gmsd, ms_gmsd, "
                         "haarpsi, msdi (formulas restated from piq / torchmetrics: parity unpinned); fsim is the only metric left out "
                         "(not on the engine: it needs 2-D FFTs of sizes the engine's FFT does not take and a per-image median)")


FSIM_ON_NOTICE = ("test: fsim (--fsim: get_fsim_metrics / get_in_fsim_metrics) computed on the MI355X engine (formula restated from piq: "
                  "parity unpinned)")
EXT_AND_FSIM_ON_NOTICE = ("test: extended metrics (get_ext_metrics / get_in_ext_metrics) and fsim (get_fsim_metrics / get_in_fsim_metrics) "
                          "computed on the MI355X engine: vif_p, gmsd, ms_gmsd, haarpsi, msdi, fsim -- the reference's whole extended set "
                          "(formulas restated from piq / torchmetrics: parity unpinned)")


def _notices(extended_metrics: bool, fsim: bool) -> list:
    """what a test epoch says about the extended metrics; without `fsim` exactly what it said before the flag existed"""
    if extended_metrics and fsim:
        return [EXT_AND_FSIM_ON_NOTICE]
    if fsim:
        return [EXT_METRICS_NOTICE, FSIM_ON_NOTICE]
    return [EXT_METRICS_ON_NOTICE if extended_metrics else EXT_METRICS_NOTICE]


def _eval_epoch(model: Model, dm, stage: str, per_rank: int, epoch: int) -> dict:
    """one validation / test epoch over this rank's shard (reference model.py:53-66 + _on_epoch_end); states are reduced over
    the ranks, so every rank returns the global values"""
    if stage == "val":
        model.on_validation_start()
    for idx in dm.batches(stage, per_rank, epoch):
        batch = dm.dataset.batch(idx, epoch)
        model.validation_step(batch) if stage == "val" else model.test_step(batch)
    return model.on_validation_epoch_end() if stage == "val" else model.on_test_epoch_end()


def _print_logged(title: str, logged: dict) -> None:
    print(f"{title}: " + ", ".join(f"{k} {float(v):.6f}" for k, v in sorted(logged.items())), flush=True)


def _fit_dataset(name, batch_size, dev, rank, world, checkpoint, seed, math, log_every, loss, scaling, dcfg, epochs, splits,
                 max_pool_bytes, extended_metrics=False, fsim=False):
    from xmm_superres_denoise.data.datamodule import XmmDataModule
    from xmm_superres_denoise.utils import Loss, create_loss, load_loss_config
    cfg = model_cfg(name, batch_size=batch_size)
    torch.manual_seed(seed)
    splits = splits or os.path.join(os.path.dirname(os.path.abspath(checkpoint)) if checkpoint else os.getcwd(),
                                    f"{dcfg.name}_{dcfg.type}_{dcfg.mode}_splits.json")
    if rank == 0:       # the first run writes the split file; the other ranks read it
        XmmDataModule(dcfg, splits, seed=seed).prepare_data()
    if dist.is_initialized():
        dist.barrier()
    dm = XmmDataModule(dcfg, splits, seed=seed, rank=rank, world=world).setup("fit", device=dev, max_pool_bytes=max_pool_bytes)
    loss_fn = create_loss(*load_loss_config(scaling)) if loss != "l1" else None
    metrics, in_metrics = _metric_sets(dcfg, "val")
    model = Model(cfg, (dcfg.lr.res, dcfg.lr.res), (dcfg.hr.res, dcfg.hr.res),
                  loss=loss_fn if loss_fn is not None else Loss({"l1": 1.0}), metrics=metrics, extended_metrics=None,
                  in_metrics=in_metrics, in_extended_metrics=None)
    model.configure_model()
    model.to(dev)
    if math:
        model.model.set_math(math)
    trainer = DataParallelTrainer(model.model, lr=cfg.optimizer.learning_rate, betas=cfg.optimizer.betas, loss=loss_fn)
    per_rank = batch_size // world if batch_size % world == 0 else batch_size
    if rank == 0 and log_every:
        print(f"dataset {dcfg.directory}/{dcfg.name}: {dm.dataset.dataset_size} samples, split "
              + " / ".join(f"{s} {len(dm.samples[s])}" for s in ("train", "val", "test"))
              + f", pool {dm.dataset.pool_bytes / 2**20:.1f} MiB, splits {splits}", flush=True)
    losses, history, best, best_state = [], [], None, None
    for epoch in range(epochs):
        ep = []
        for idx in dm.batches("train", per_rank, epoch):
            lr_img, hr_img = dm.dataset.batch(idx, epoch)
            ep.append(float(trainer.global_loss(trainer.train_step(lr_img, hr_img))))
        losses.extend(ep)
        logged = _eval_epoch(model, dm, "val", per_rank, epoch)
        vl = float(logged["val/loss"])
        history.append({"epoch": epoch, "train/loss": sum(ep) / max(1, len(ep)), "val/loss": vl})
        if rank == 0 and log_every:
            print(f"epoch {epoch}: train/loss {history[-1]['train/loss']:.6f} val/loss {vl:.6f}", flush=True)
        if best is None or vl < best:       # ModelCheckpoint(monitor="val/loss", mode="min")
            best = vl
            best_state = {k: v.detach().clone() for k, v in model.model.state_dict().items()}
            if checkpoint and rank == 0:
                save_checkpoint(checkpoint, model, trainer, epoch=epoch)
    # trainer.test(ckpt_path="best"): the test epoch on the best weights, with the test-prefixed metric sets
    model.model.load_state_dict(best_state)
    model.metrics, model.in_metrics = _metric_sets(dcfg, "test")
    if extended_metrics:
        model.ext_metrics, model.in_ext_metrics = _ext_metric_sets(dcfg, "test")
    if fsim:
        model.fsim_metrics, model.in_fsim_metrics = _fsim_metric_sets(dcfg, "test")
    test_logged = _eval_epoch(model, dm, "test", per_rank, 0)
    if rank == 0 and log_every:
        _print_logged(f"test (best val/loss {best:.6f})", test_logged)
        print("\n".join(_notices(extended_metrics, fsim)), flush=True)
    model.history, model.test_logged = history, test_logged
    return model, trainer, losses


def test(checkpoint: str, dataset_dir: str, name: str = "rrdb_denoise", dataset_name: str = "sim_dataset",
         dataset_type: str = "sim", lr_res: int = 416, lr_exps=(20,), hr_exp: int = 100, lr_det_mask=None, hr_det_mask=None,
         agn: int = 1, lr_bkg: int = 1, comb_hr: bool = False, scaling: str = "linear", batch_size: int = 4, loss: str = "l1",
         seed: int | None = None, splits: str | None = None, device: str | None = None, max_pool_bytes: int | None = None,
         log: bool = True, extended_metrics: bool = False, math: str | None = None, fsim: bool = False, dim: int | None = None) -> dict:
    """The reference's `train.py test` (train.py:91-103,165-171) on one device: the test split of the dataset through the model
    of `checkpoint` (any model infer.load_model loads), returning the `test/...` values (loss, get_metrics, get_in_metrics).
    The split file must be the one `fit` wrote (default location: next to the checkpoint); `seed` defaults to the one recorded
    there, so the test samples draw the same realisations, AGN and backgrounds as fit's test epoch.  Without `extended_metrics` the
    extended piq / VIF collection is not computed and the routine says so (EXT_METRICS_NOTICE) instead of leaving it out silently; with
    it, get_ext_metrics / get_in_ext_metrics (vif_p, gmsd, ms_gmsd, haarpsi, msdi) are added and the notice names fsim as the one
    metric left out.  `fsim` adds get_fsim_metrics / get_in_fsim_metrics (test/<mode>/fsim, test/<mode>/in/fsim; parity unpinned) for any of
    the five models, with or without `extended_metrics`, and says so (FSIM_ON_NOTICE, or one combined notice when both are given).
    `math` is infer.load_model's: the math mode of the network (None: its default); so is `dim`, Restormer's width (None: 24 of
    models.toml), refused with any other model before anything is read."""
    from xmm_superres_denoise.data.datamodule import XmmDataModule
    from xmm_superres_denoise.infer import check_dim, load_model
    check_dim(name, dim)
    from xmm_superres_denoise.utils import Loss, create_loss, load_loss_config
    if torch.cuda.device_count() < 1:
        raise RuntimeError("train.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    dev = torch.device(device or "cuda:0")
    torch.cuda.set_device(dev)
    dcfg = dataset_cfg(dataset_dir, dataset_name, dataset_type, name, lr_res, lr_exps, hr_exp, lr_det_mask, hr_det_mask, agn,
                       lr_bkg, comb_hr, scaling, batch_size)
    splits = splits or os.path.join(os.path.dirname(os.path.abspath(checkpoint)), f"{dcfg.name}_{dcfg.type}_{dcfg.mode}_splits.json")
    if not os.path.exists(splits):
        raise FileNotFoundError(f"{splits}: no split file (fit writes it next to its checkpoint; pass splits= to name another)")
    if seed is None:
        import json
        with open(splits) as f:
            seed = int(json.load(f).get("seed", 0))
    dm = XmmDataModule(dcfg, splits, seed=seed).setup("test", device=dev, max_pool_bytes=max_pool_bytes)
    model = load_model(checkpoint, name, lr_res, device=dev, math=math, dim=dim)
    model.loss = create_loss(*load_loss_config(scaling)) if loss != "l1" else Loss({"l1": 1.0})
    model.metrics, model.in_metrics = _metric_sets(dcfg, "test")
    if extended_metrics:
        model.ext_metrics, model.in_ext_metrics = _ext_metric_sets(dcfg, "test")
    if fsim:
        model.fsim_metrics, model.in_fsim_metrics = _fsim_metric_sets(dcfg, "test")
    with torch.no_grad():
        logged = _eval_epoch(model, dm, "test", batch_size, 0)
    logged = {k: float(v) for k, v in logged.items()}
    if log:
        _print_logged("test", logged)
        print("\n".join(_notices(extended_metrics, fsim)), flush=True)
    return logged


def main():
    ap = argparse.ArgumentParser(description="fit an RRDB generator with the MI355X engine, on random tiles or an XMM FITS dataset; "
                                             "test a checkpoint on a dataset's test split")
    ap.add_argument("routine", choices=["fit", "test"])
    ap.add_argument("--model", default="rrdb_denoise", choices=["rrdb_denoise", "esr_gen", "restormer", "swinfir", "hat"],
                    help="fit refuses restormer, swinfir and hat: forward only on this engine; test takes all five")
    ap.add_argument("--lr-res", type=int, default=416)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--math", default=None, choices=[None, "fp32", "bf16x6", "f16x3"])
    ap.add_argument("--dim", type=int, default=None,
                    help="test --model restormer: the network's width (default: 24 of models.toml; 48 is the published Restormer)")
    ap.add_argument("--loss", default="l1", choices=["l1", "paper"], help="paper = 0.5 psnr + 0.5 ms_ssim (loss_functions.toml)")
    ap.add_argument("--scaling", default="linear", choices=["linear", "sqrt", "asinh", "log"])
    ap.add_argument("--val-batches", type=int, default=0, help="validation batches after training (loss + metric set)")
    ap.add_argument("--dataset-dir", default=None, help="train / test on the FITS tree <dir>/<dataset-name>/... (default: random tiles)")
    ap.add_argument("--dataset-name", default="sim_dataset")
    ap.add_argument("--dataset-type", default="sim", choices=["sim", "real"])
    ap.add_argument("--lr-exps", type=int, nargs="+", default=[20])
    ap.add_argument("--hr-exp", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--lr-det-mask", default=None)
    ap.add_argument("--hr-det-mask", default=None)
    ap.add_argument("--agn", type=int, default=1)
    ap.add_argument("--lr-bkg", type=int, default=1)
    ap.add_argument("--comb-hr", action="store_true")
    ap.add_argument("--splits", default=None, help="split JSON (default: next to the checkpoint)")
    ap.add_argument("--seed", type=int, default=None, help="fit: default 0; test: default the seed recorded in the split file")
    ap.add_argument("--extended-metrics", action="store_true",
                    help="test (and fit's final test epoch): add vif_p, gmsd, ms_gmsd, haarpsi, msdi (get_ext_metrics / get_in_ext_metrics; no fsim)")
    ap.add_argument("--fsim", action="store_true",
                    help="test (and fit's final test epoch): add fsim as test/<mode>/fsim and test/<mode>/in/fsim (parity unpinned); "
                         "independent of --extended-metrics")
    a = ap.parse_args()
    if a.routine == "test" and a.model == "restormer" and a.math not in (None, "fp32"):
        ap.error(f"restormer: math mode {a.math!r} is not supported: the Restormer engine computes in 'fp32' only")
    if a.dim is not None and (a.routine != "test" or a.model != "restormer"):
        ap.error(f"{a.model}: --dim {a.dim} is not supported: dim is the width of `test --model restormer` only")
    ds = dict(dataset_name=a.dataset_name, dataset_type=a.dataset_type, lr_exps=tuple(a.lr_exps), hr_exp=a.hr_exp,
              lr_det_mask=a.lr_det_mask, hr_det_mask=a.hr_det_mask, agn=a.agn, lr_bkg=a.lr_bkg, comb_hr=a.comb_hr, splits=a.splits)
    if a.routine == "test":
        if not a.checkpoint or not a.dataset_dir:
            ap.error("test needs --checkpoint and --dataset-dir")
        test(a.checkpoint, a.dataset_dir, name=a.model, lr_res=a.lr_res, scaling=a.scaling, batch_size=a.batch_size, loss=a.loss,
             seed=a.seed, extended_metrics=a.extended_metrics, math=a.math, fsim=a.fsim, dim=a.dim, **ds)
    elif a.dataset_dir is None:
        fit(a.model, a.lr_res, a.batch_size, a.steps, checkpoint=a.checkpoint, math=a.math, loss=a.loss, scaling=a.scaling, val_batches=a.val_batches)
    else:
        fit(a.model, a.lr_res, a.batch_size, a.steps, checkpoint=a.checkpoint, math=a.math, loss=a.loss, scaling=a.scaling,
            seed=0 if a.seed is None else a.seed, dataset_dir=a.dataset_dir, epochs=a.epochs, extended_metrics=a.extended_metrics, fsim=a.fsim, **ds)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
