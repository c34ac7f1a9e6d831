"""TrainableSwinFIR: the reference's SwinFIR forward (models/transformer/swinfir.py:120-441 with the Swin blocks of modules.py) for
upsampler "pixelshuffle" and resi_connection "1conv", composed in Python from the differentiable ops of xmm_superres_denoise/ops.py
(hand-written HIP forward and backward: linear, conv3x3, layer_norm, window_attention), with torch's autograd holding the graph.
Plain torch ops do the plumbing only: the mean / img_range affine, residual adds, reshapes / transposes, pixel_shuffle, DropPath's
per-sample scale, the optional clamp.

It WRAPS a models.SwinFIR and shares its Parameter objects exactly as TrainableSwinIR wraps a models.SwinIR: state-dict key names,
order, init and checkpoints are the reference's (the wrapper's state_dict / load_state_dict are the wrapped module's), and after
training the wrapped module's fused forward (csrc/swinfir.hip) re-packs and sees the new weights.  models.SwinFIR itself stays
forward-only and keeps its refusal.

Refused in the constructor, by name: resi_connection "SFB" (the FourierUnit's rfftn / irfftn pair has no differentiable op on the
engine; its forward runs through models.SwinFIR) and dropout rates other than 0.
Window size and shift are each block's own (`blk.window_size`, `blk.shift_size`): where img_size // patch_size <= window_size the
reference clamps the window and drops the shift.  models.SwinFIR pads nothing, so sizes off the window grid are refused in the wrapped
module's own words.

DropPath, `generator`, `last_drop_masks`, `clamp`, the RSTB loop and the pixel-shuffle tail are TrainableSwinIR's, in one copy
(swinir_train.py: TrainableSwin).  The RSTB's closing conv is outside every
dropped branch: a sample whose Swin branches were all dropped still sends it a gradient.
"""
from __future__ import annotations

import torch

from xmm_superres_denoise.engine import XsdError

from .swinfir import SwinFIR
from .swinir_train import TrainableSwin


class TrainableSwinFIR(TrainableSwin):
    def __init__(self, module: SwinFIR, drop_path_rate: float | None = None, generator: torch.Generator | None = None,
                 clamp: bool = False):
        """`drop_path_rate`: None takes the wrapped module's constructor argument.  `clamp`: clamp the output to [0, 1] as Model.forward
        does (models/model.py:48-49)."""
        super().__init__()
        if not isinstance(module, SwinFIR):
            raise TypeError(f"TrainableSwinFIR wraps a models.SwinFIR (got {type(module).__name__})")
        if module.resi_connection != "1conv":
            raise NotImplementedError(f"TrainableSwinFIR: resi_connection {module.resi_connection!r} is not trainable on the MI355X engine "
                                      "(trainable: \"1conv\"; the FourierUnit of the SFB has no differentiable FFT op); its forward runs "
                                      "through models.SwinFIR")
        self._wrap(module, drop_path_rate, generator, clamp)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        m = self.module
        self._check_input(x)
        H, W = int(x.shape[2]), int(x.shape[3])
        # the sizes models.SwinFIR.forward refuses, in its words
        if H % m.window or W % m.window:
            raise XsdError(f"SwinFIR needs H and W that are multiples of the window size {m.window} (window_partition, "
                           f"modules.py); got {H} x {W}")
        self.last_drop_masks = []
        mean = self._mean_like(x)
        y = self._pixelshuffle_tail(self._features((x - mean) * m.img_range))      # each block's own window: the clamped case
        y = (y / m.img_range + mean).contiguous()
        return y.clamp(0.0, 1.0) if self.clamp else y
