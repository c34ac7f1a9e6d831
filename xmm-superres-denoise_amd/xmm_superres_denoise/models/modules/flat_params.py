"""What the engine-backed modules share (GeneratorRRDB_DN / _SR, Restormer, SwinFIR, HAT, SwinIR): the flat parameter buffer the engines
read (include/xsd.h: "flat params": every parameter a view into one contiguous fp32 buffer in state_dict order), the engine handle, the
pack rule (every forward packs: torch's version counters miss the writes made through `.data`), the version sum a
recomputing backward compares, the math mode, the copy / pickle rule, the input checks and the one forward-only autograd function.  A
module provides _make_engine, its constructor checks and its forward's size rule."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from xmm_superres_denoise.engine import XsdError


def tracks_version(t: torch.Tensor) -> bool:
    """False for a tensor born under torch.inference_mode(), also after its .data was pointed elsewhere (is_inference() is then False)"""
    try:
        t._version
    except RuntimeError:
        return False
    return True


def inference_refusal(name: str, whose: str) -> RuntimeError:
    """What a forward that a backward may follow answers when the parameters were created under torch.inference_mode().  Such
    parameters stay without a version counter for good: pointing their .data at a normal tensor (flatten_parameters does) makes
    is_inference() answer False and changes nothing else -- reading `_version` raises, and so does any autograd op that would save
    them.  Forwards without a graph run on them."""
    return RuntimeError(f"{name}: {whose} parameters are inference tensors (built or loaded under torch.inference_mode()), which autograd "
                        "cannot train; forwards under torch.no_grad() / inference_mode() work, for training build the module outside "
                        "inference mode")


class _ForwardOnlyFn(torch.autograd.Function):
    """The forward of a module without a backward on the engine: works in any grad mode; a backward that reaches it is refused by name.
    It packs on every call, as the RRDB generators' forward does, and reads no version counter: parameters that are inference tensors
    (a module built under torch.inference_mode()) have none."""

    @staticmethod
    def forward(ctx, module, x, *params):
        ctx.network = module.NETWORK
        eng = module._get_engine(x.device)
        eng.pack(module._flat)
        return eng.forward(x.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        raise RuntimeError(f"{ctx.network} training is not on the MI355X engine: its backward is not implemented (forward only: "
                           "inference, infer.py, validation / test metrics)")


class FlatParams:
    """Base of an nn.Module that computes through an engine.  A subclass names its engine class (ENGINE: its MATH table lists the math
    modes) and its network (NETWORK), calls _init_engine_state() at the end of __init__ and provides _make_engine()."""

    ENGINE = None
    NETWORK = ""
    DEFAULT_MATH = "fp32"       # what get_math answers before set_math; None: the engine's own default, known once an engine exists

    def _init_engine_state(self):
        self._engine = None
        self._engine_dev = None
        self._flat = None
        self._plist = None
        self._math = None       # None: the engine's default

    # ---- copies and pickles (copy.deepcopy for EMA / SWA copies, torch.save(module), spawn-style launchers) --------------------
    def __getstate__(self):
        """The engine handle belongs to this process and this module: a copy or an unpickled module builds its own (and lays its own
        flat parameter buffer, and packs) at its first forward, exactly like a freshly constructed one.  The math mode is carried."""
        st = self.__dict__.copy()
        st["_engine"] = st["_engine_dev"] = st["_flat"] = st["_plist"] = None
        return st

    # ---- math mode -----------------------------------------------------------------------------------------------------------------
    def _math_refusal(self, mode: str) -> Exception:
        return ValueError(f"{self.NETWORK}: math mode {mode!r} is not supported; the modes are {sorted(self.ENGINE.MATH)}"
                          + (" (the fp16 terms of 'f16x3' need a per-tensor scale that these kernels do not publish)" if mode == "f16x3" else ""))

    def set_math(self, mode: str):
        """Math mode of the engine's matrix kernels (ENGINE.set_math; ENGINE.MATH lists the modes).  Kept until an engine exists, applied
        again to the engine a device move creates, and carried by copies and pickles."""
        if mode not in self.ENGINE.MATH:
            raise self._math_refusal(mode)
        self._math = mode
        if self._engine is not None:
            self._engine.set_math(mode)
        return self

    def get_math(self) -> str:
        return getattr(self, "_math", None) or self.DEFAULT_MATH

    # ---- engine --------------------------------------------------------------------------------------------------------------------
    def _make_engine(self):
        """the one ENGINE(...) call, from the module's constructor arguments"""
        raise NotImplementedError

    def _get_engine(self, device):
        if not torch.device(device).type == "cuda":
            raise XsdError("the MI355X engine needs CUDA(HIP) tensors; there is no CPU fallback")
        flat = self.flatten_parameters()
        if flat.device != torch.device(device):
            raise XsdError(f"module parameters are on {flat.device} but the input is on {device}")
        if self._engine is None or self._engine_dev != flat.device:
            with torch.cuda.device(flat.device):
                self._engine = self._make_engine()
            self._engine_dev = flat.device
            if getattr(self, "_math", None) is not None:
                self._engine.set_math(self._math)
        return self._engine

    # ---- forward -------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_input(x: torch.Tensor, channels: int | None):
        """`channels`: None leaves the shape to the engine"""
        if x.dtype != torch.float32:
            raise XsdError(f"input must be float32 (got {x.dtype})")
        if channels is not None and (x.dim() != 4 or x.shape[1] != channels):
            raise XsdError(f"input must be [B,{channels},H,W] (got {tuple(x.shape)})")

    def _forward_only(self, x: torch.Tensor, channels: int, Ho: int, Wo: int):
        """x through the engine's forward -> [B, channels, Ho, Wo]"""
        self._get_engine(x.device)
        if x.shape[0] == 0:      # an empty batch answers like torch's convs: empty output, no launch
            return x.new_empty((0, channels, Ho, Wo))
        return _ForwardOnlyFn.apply(self, x, *self._plist)

    # ---- flat parameter buffer ---------------------------------------------------------------------------------
    def flatten_parameters(self):
        """Make every parameter a view into ONE contiguous fp32 buffer in state_dict order (the engine's flat-params
        layout, include/xsd.h).  Re-run automatically after .to()/.cuda() moved the parameters."""
        plist = list(self.parameters())
        dev = plist[0].device
        ok = self._flat is not None and self._flat.device == dev
        if ok:
            off = 0
            base = self._flat.data_ptr()
            for p in plist:
                if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                    ok = False
                    break
                off += p.numel()
        if not ok:
            # The first forward of a Lightning run is a validation sanity check under torch.inference_mode(): a buffer made there would be
            # an inference tensor and the parameters views of it -- no optimizer could ever update them.  Make it a normal tensor.
            with torch.inference_mode(False):
                flat = torch.empty(sum(p.numel() for p in plist), dtype=torch.float32, device=dev)
                off = 0
                for p in plist:
                    n = p.numel()
                    flat[off:off + n].copy_(p.data.reshape(-1).float())
                    p.data = flat[off:off + n].view(p.shape)
                    off += n
            self._flat = flat
        self._plist = plist
        return self._flat

    def flat_parameters(self) -> torch.Tensor:
        return self.flatten_parameters()

    def _param_version(self) -> int:
        """Changes with every in-place update torch knows of: the parameters keep their OWN version counters when their .data is
        pointed into the flat buffer (an optimizer step, load_state_dict or an in-place op on the parameter bumps the parameter's, an
        update of the flat buffer itself -- the fused Adam of parallel.py goes through a raw pointer and is sequenced by its caller --
        the buffer's).  It does NOT change with a write through `.data` (`p.data.mul_()`, the EMA idiom, `w.data.normal_()`): torch
        bumps no counter for those, so nothing that must see every write may rest on this sum -- the packed copies do not (every
        forward packs).  Read only where a backward can follow: its one user is the recomputing backward's guard, which shares the
        blind spot with torch's own saved-tensor check.  Inference-tensor parameters have no counter and are refused by name."""
        try:
            return self._flat._version + sum(p._version for p in self._plist)
        except RuntimeError as e:       # torch's bare "Inference tensors do not track version counter"
            raise inference_refusal(type(self).__name__, "the") from e
