"""Validation metric set of the reference (metrics/xmm_metric_collection.py:14-38,67-91,114-143): psnr, ssim, ms_ssim
(kernel_size=13, sigma=2.5, k2=0.05), l1, l2, poisson, evaluated once per scaling normalizer ("linear", "sqrt", ...)
on images whose dataset stretch is first undone and which are then re-stretched with that normalizer.

All values come from one `xsd_loss_eval` call per (batch, stretch mode) (include/xsd.h); the per-batch states it returns
(sum of squared errors, target range, per-image similarity sums) are accumulated on the device exactly as the
torchmetrics classes accumulate theirs, so `compute()` gives epoch-level values, not a mean of batch values:
  psnr    10*log10(data_range^2 / (sum_sq_err / n)), data_range = max(target) - min(target) over the epoch with both
          states starting at 0 (PeakSignalNoiseRatio(data_range=None));
  ssim / ms_ssim   sum of per-image values / number of images;
  l1, l2  sum of absolute / squared errors / n;
  poisson sum of per-batch means / number of images (metrics/metrics.py:30-39 as written).
`denorm` / `norm` are the bare stretch functions of Normalize (transforms/normalize.py:55-62), applied to [0,1] images as
in the reference's `update` (:136-143).

The "extended" collections of the reference's `test` (get_ext_metrics / get_in_ext_metrics, :41-61,91-111) are XMMExtMetricCollection:
vif_p, gmsd, ms_gmsd, haarpsi, msdi from one `xsd_ext_metrics_eval` per (batch, stretch mode), which returns per-image doubles; the
reference's reductions (metrics/metrics.py:9-27) happen here, on the device, in double:
  gmsd, ms_gmsd, haarpsi, msdi   sum of per-batch MEANS / number of images (the piq wrappers add the batch mean to `metric` and the
          batch size to `total`: the quirk `poisson` shows too);
  vif_p   torchmetrics' own class: sum of per-image values / number of images.
Their formulas restate piq 0.7.x / torchmetrics 1.x from the published code: parity with the libraries is unpinned (INTEGRATION.md
section 3).  XMMExtMetricCollection refuses fsim by name (that refusal is pinned by tests); fsim is an opt-in collection of its own,
XMMFsimCollection (get_fsim_metrics / get_in_fsim_metrics): one `xsd_fsim_eval` per (batch, stretch mode), the same `_Metric` reduction
(sum of per-batch means / number of images), piq's formula restated in tests/golden/fsim_torch.py -- parity unpinned as well.
"""
from __future__ import annotations

from typing import List

import torch

from ..utils.loss_functions import EpochState, Loss

NAMES = ("psnr", "ssim", "ms_ssim", "l1", "l2", "poisson")


class XMMMetricCollection:
    """reference signature: XMMMetricCollection(metrics, dataset_normalizer, scaling_normalizers, prefix); `metrics` is the
    tuple of metric names (optionally prefixed, e.g. "in/psnr") instead of a torchmetrics MetricCollection."""

    def __init__(self, metrics, dataset_normalizer, scaling_normalizers: List, prefix: str):
        self.names = tuple(metrics)
        for n in self.names:
            if n.split("/")[-1] not in NAMES:
                raise NotImplementedError(f"metric {n}: only {NAMES} run on the MI355X engine (SURVEY.md section 8f-4)")
        self.dataset_normalizer = dataset_normalizer
        self.normalizer_dict = {n.stretch_mode: n for n in scaling_normalizers}
        self.prefix = prefix
        self._eval = Loss({"l1": 1.0, "poisson": 1.0, "psnr": 1.0, "ssim": 1.0, "ms_ssim": 1.0})
        self.reset()

    def reset(self):
        self.states = {mode: EpochState() for mode in self.normalizer_dict}

    @torch.no_grad()
    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        preds = self.dataset_normalizer.denorm(preds)
        target = self.dataset_normalizer.denorm(target)
        nimg = preds.shape[0]
        for mode, normalizer in self.normalizer_dict.items():
            p = normalizer.norm(preds).contiguous()
            t = normalizer.norm(target).contiguous()
            out, _ = self._eval._eval(p, t, False)
            self.states[mode].add(out, p.numel(), nimg)

    def sync(self, group=None) -> None:
        """all-reduce the per-mode epoch states over the ranks (sum / min / max), see EpochState.sync"""
        for st in self.states.values():
            st.sync(group)

    def compute(self) -> dict:
        res = {}
        for mode, st in self.states.items():
            vals = st.compute()
            for n in self.names:
                head, _, base = n.rpartition("/")
                key = f"{self.prefix}/{mode}/{n}"
                res[key] = vals[base].float()
        return res


EXT_NAMES = ("vif_p", "gmsd", "ms_gmsd", "haarpsi", "msdi")
FSIM_REFUSAL = ("fsim is not on the MI355X engine: its phase congruency needs 2-D FFTs of the pooled image (278 = 2 * 139 points a side "
                "for 832 x 832 tiles; the engine's FFT takes prime factors up to 13) and a per-image median")


class ExtEpochState:
    """Epoch states of the reference's extended metrics, double, on the device of the values: [gmsd, ms_gmsd, haarpsi, msdi] sums of
    per-batch means, the sum of per-image vif_p, the number of images."""

    def __init__(self):
        self.acc = None

    def add(self, per_image: torch.Tensor) -> None:
        """per_image: [B, 6] float64 of one batch (gmsd, ms_gmsd, haarpsi, mdsi, vif numerator, vif denominator per image)"""
        v = per_image.double()
        cur = torch.cat([v[:, :4].mean(0), (v[:, 4] / v[:, 5]).sum().reshape(1), v.new_tensor([float(v.shape[0])])])
        self.acc = cur if self.acc is None else self.acc + cur

    def sync(self, group=None, device=None) -> None:
        """sum the states over the ranks (dist_reduce_fx="sum" of every state, metrics/metrics.py:16-21); a rank that saw no batch
        takes part with zeros, see EpochState.sync"""
        import torch.distributed as dist
        from xmm_superres_denoise.parallel import all_reduce_any, collectives_on
        if not collectives_on(group):
            return
        if self.acc is not None:
            a = self.acc.clone()
        else:
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
            a = torch.zeros(6, dtype=torch.float64, device=device)
        all_reduce_any(a, dist.ReduceOp.SUM, group)
        self.acc = None if float(a[5]) == 0.0 else a

    def compute(self) -> dict:
        a = self.acc
        return {"gmsd": a[0] / a[5], "ms_gmsd": a[1] / a[5], "haarpsi": a[2] / a[5], "msdi": a[3] / a[5], "vif_p": a[4] / a[5]}


class XMMExtMetricCollection:
    """The reference's XMMMetricCollection over its extended metric set: same constructor, same denorm -> renorm per scaling
    normaliser, keys "<prefix>/<mode>/<name>"."""

    def __init__(self, metrics, dataset_normalizer, scaling_normalizers: List, prefix: str):
        self.names = tuple(metrics)
        for n in self.names:
            base = n.split("/")[-1]
            if base == "fsim":
                raise NotImplementedError(f"metric {n}: {FSIM_REFUSAL}")
            if base not in EXT_NAMES:
                raise NotImplementedError(f"metric {n}: the extended set on the MI355X engine is {EXT_NAMES}")
        self.dataset_normalizer = dataset_normalizer
        self.normalizer_dict = {n.stretch_mode: n for n in scaling_normalizers}
        self.prefix = prefix
        self._engines = {}       # one engine (device workspace) per device
        self.reset()

    def reset(self):
        self.states = {mode: ExtEpochState() for mode in self.normalizer_dict}

    def _engine(self, device):
        from ..engine.engine import ExtMetricsEngine
        if device.index not in self._engines:
            with torch.cuda.device(device):
                self._engines[device.index] = ExtMetricsEngine()
        return self._engines[device.index]

    @torch.no_grad()
    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if preds.dim() != 4 or preds.shape[1] != 1:
            raise NotImplementedError(f"extended metrics: only single-channel [B, 1, H, W] images run on the MI355X engine (got "
                                      f"{tuple(preds.shape)}; piq's RGB / YIQ branches are not built)")
        preds = self.dataset_normalizer.denorm(preds)
        target = self.dataset_normalizer.denorm(target)
        for mode, normalizer in self.normalizer_dict.items():
            p = normalizer.norm(preds).contiguous()
            t = normalizer.norm(target).contiguous()
            self.states[mode].add(self._engine(p.device).eval(p, t))

    def sync(self, group=None) -> None:
        for st in self.states.values():
            st.sync(group)

    def compute(self) -> dict:
        res = {}
        for mode, st in self.states.items():
            vals = st.compute()
            for n in self.names:
                res[f"{self.prefix}/{mode}/{n}"] = vals[n.rpartition("/")[2]].float()
        return res


class FsimEpochState:
    """Epoch state of the reference's `_Metric` wrapper around piq.fsim (metrics/metrics.py:9-27,92-101), double, on the device of the
    values: [sum of per-batch means, number of images]."""

    def __init__(self):
        self.acc = None

    def add(self, per_image: torch.Tensor) -> None:
        """per_image: [B] float64 of one batch: the BATCH MEAN goes to `metric`, B to `total`"""
        v = per_image.double()
        cur = torch.stack([v.mean(), v.new_tensor(float(v.shape[0]))])
        self.acc = cur if self.acc is None else self.acc + cur

    def sync(self, group=None, device=None) -> None:
        """sum both states over the ranks; a rank that saw no batch takes part with zeros (see ExtEpochState.sync)"""
        import torch.distributed as dist
        from xmm_superres_denoise.parallel import all_reduce_any, collectives_on
        if not collectives_on(group):
            return
        if self.acc is not None:
            a = self.acc.clone()
        else:
            if device is None:
                device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
            a = torch.zeros(2, dtype=torch.float64, device=device)
        all_reduce_any(a, dist.ReduceOp.SUM, group)
        self.acc = None if float(a[1]) == 0.0 else a

    def compute(self) -> torch.Tensor:
        return self.acc[0] / self.acc[1]


class XMMFsimCollection:
    """fsim beside XMMExtMetricCollection (which keeps refusing it by name): the same denorm -> renorm per scaling normaliser, keys
    "<prefix>/<mode>/fsim" or, with `input_side`, "<prefix>/<mode>/in/fsim".  The formula restates piq 0.7.x fsim(chromatic=False) from its
    published code: parity with piq is unpinned."""

    def __init__(self, dataset_normalizer, scaling_normalizers: List, prefix: str, input_side: bool = False):
        self.name = "in/fsim" if input_side else "fsim"
        self.dataset_normalizer = dataset_normalizer
        self.normalizer_dict = {n.stretch_mode: n for n in scaling_normalizers}
        self.prefix = prefix
        self._engines = {}       # one engine (device workspace + plans) per device
        self.reset()

    def reset(self):
        self.states = {mode: FsimEpochState() for mode in self.normalizer_dict}

    def _engine(self, device):
        from ..engine.engine import FsimEngine
        if device.index not in self._engines:
            with torch.cuda.device(device):
                self._engines[device.index] = FsimEngine()
        return self._engines[device.index]

    @torch.no_grad()
    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        if preds.dim() != 4 or preds.shape[1] != 1:
            raise NotImplementedError(f"fsim: only single-channel [B, 1, H, W] images run on the MI355X engine (got {tuple(preds.shape)}; "
                                      "piq's chromatic / YIQ branch is not built)")
        preds = self.dataset_normalizer.denorm(preds)
        target = self.dataset_normalizer.denorm(target)
        for mode, normalizer in self.normalizer_dict.items():
            p = normalizer.norm(preds).contiguous()
            t = normalizer.norm(target).contiguous()
            self.states[mode].add(self._engine(p.device).eval(p, t))

    def sync(self, group=None) -> None:
        for st in self.states.values():
            st.sync(group)

    def compute(self) -> dict:
        return {f"{self.prefix}/{mode}/{self.name}": st.compute().float() for mode, st in self.states.items()}


def get_metrics(dataset_normalizer, scaling_normalizers: List, prefix: str) -> XMMMetricCollection:
    return XMMMetricCollection(NAMES, dataset_normalizer, scaling_normalizers, prefix)


def get_in_metrics(dataset_normalizer, scaling_normalizers: List, prefix: str) -> XMMMetricCollection:
    return XMMMetricCollection(tuple("in/" + n for n in NAMES), dataset_normalizer, scaling_normalizers, prefix)


def get_ext_metrics(dataset_normalizer, scaling_normalizers: List, prefix: str) -> XMMExtMetricCollection:
    """the reference's get_ext_metrics without fsim (refused by name when asked for: XMMExtMetricCollection)"""
    return XMMExtMetricCollection(EXT_NAMES, dataset_normalizer, scaling_normalizers, prefix)


def get_in_ext_metrics(dataset_normalizer, scaling_normalizers: List, prefix: str) -> XMMExtMetricCollection:
    return XMMExtMetricCollection(tuple("in/" + n for n in EXT_NAMES), dataset_normalizer, scaling_normalizers, prefix)


def get_fsim_metrics(dataset_normalizer, scaling_normalizers: List, prefix: str) -> XMMFsimCollection:
    """the `fsim` entry of the reference's get_ext_metrics, as a collection of its own (opt-in: train --fsim)"""
    return XMMFsimCollection(dataset_normalizer, scaling_normalizers, prefix)


def get_in_fsim_metrics(dataset_normalizer, scaling_normalizers: List, prefix: str) -> XMMFsimCollection:
    return XMMFsimCollection(dataset_normalizer, scaling_normalizers, prefix, input_side=True)
