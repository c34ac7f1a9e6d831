"""The flat parameter buffer the engines read (include/xsd.h: "flat params"), shared by the generator modules: every parameter a
view into one contiguous fp32 buffer in state_dict order, the version counter that says when it changed, and the copy / pickle
rule for the engine handle."""
from __future__ import annotations

import torch


class FlatParams:
    """Mixin for an nn.Module with the attributes _engine, _engine_dev, _flat and _plist."""

    # ---- copies and pickles (copy.deepcopy for EMA / SWA copies, torch.save(module), spawn-style launchers) --------------------
    def __getstate__(self):
        """The engine handle belongs to this process and this module: a copy or an unpickled module builds its own (and lays its own
        flat parameter buffer) at its first forward, exactly like a freshly constructed one."""
        st = self.__dict__.copy()
        st["_engine"] = st["_engine_dev"] = st["_flat"] = st["_plist"] = None
        return st

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
        pointed into the flat buffer (an optimizer step or load_state_dict bumps the parameter's, an update of the flat buffer itself
        -- the fused Adam of parallel.py goes through a raw pointer and is sequenced by its caller -- the buffer's)."""
        return self._flat._version + sum(p._version for p in self._plist)
