"""What torch does to a parameter that FlatParams.flatten_parameters (models/modules/flat_params.py) laid into a flat buffer, for every
way torch code rewrites parameters: one case per idiom, plain torch on the CPU, no engine.  Each case pins five observations:

  flat_version   how far `flat._version` moved
  p_version      how far the parameter's own `_version` moved (None: the Parameter object was replaced)
  moved          the parameter's `data_ptr()` left its place in the buffer
  same_param     the module still holds the same Parameter object
  flat_changed   the bytes of the buffer changed

FlatParams._param_version (the sum of the two counters) rests on the rows where one of them moves, and the modules' pack rule (every
forward packs) on the rows where NEITHER moves although the bytes did: the writes through `.data` and the step of
torch's fused Adam.  A torch
upgrade that moves a row shows up here and not as a wrong image.  tests/test_hip_param_writes.py runs the same idioms through the
engines.  A device move cannot happen without a device; `to(float64).to(float32)` goes through the same nn.Module._apply and stands in
for `m.cpu()` ... `m.cuda()`."""
import copy

import pytest
import torch
from torch import nn
from torch.nn.utils import parameters_to_vector, vector_to_parameters
from torch.optim.swa_utils import AveragedModel

from xmm_superres_denoise.models.modules.flat_params import FlatParams


class _Tiny(FlatParams, nn.Module):
    """two layers, so that the observed parameter (b.weight) does not start the buffer"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = nn.Linear(2, 2)
        self.b = nn.Linear(4, 3)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g))
        self._init_engine_state()


class _Ctx:
    def __init__(self, averaged=False):
        self.other = _Tiny(1)
        self.other.flatten_parameters()
        if averaged:                      # the observed module is the averaged copy swa_utils keeps
            self.avg = AveragedModel(_Tiny(0))
            self.m = self.avg.module
        else:
            self.m = _Tiny(0)
        self.flat = self.m.flatten_parameters()
        self.p = self.m.b.weight
        self.w = torch.full((3, 4), 0.25)


def _set_grads(m):
    for i, p in enumerate(m.parameters()):
        p.grad = torch.full_like(p, 0.5 + i)


def _step(make):
    def write(c):
        _set_grads(c.m)
        make(c.m.parameters()).step()
    return write


def _ema(c, decay=0.5):                   # BasicSR's model_ema: net_g_ema_params[k].data.mul_(decay).add_(net_g_params[k].data, alpha=1 - decay)
    for ema_p, p in zip(c.m.parameters(), c.other.parameters()):
        ema_p.data.mul_(decay).add_(p.data, alpha=1 - decay)


def _init_fn(mod):
    if isinstance(mod, nn.Linear):
        mod.weight.data.normal_()


def _nograd(fn):
    def write(c):
        with torch.no_grad():
            fn(c)
    return write


def _inference_data_write(c):
    with torch.inference_mode():
        c.p.data.mul_(2)


def _swa(c):
    c.avg.update_parameters(c.other)      # the first one copies (p_averaged.detach().copy_(p_model)) ...
    with torch.no_grad():
        for p in c.other.parameters():
            p.add_(1.0)
    c.avg.update_parameters(c.other)      # ... the second one averages


def _vector(c):
    vector_to_parameters(0.5 * parameters_to_vector(c.m.parameters()), c.m.parameters())


def _rebind(c):
    c.p.data = c.w.clone()


WRITES = {
    # ---- through .data: the bytes change and torch bumps NOTHING ------------------------------------------------------------------
    "p.data.mul_": lambda c: c.p.data.mul_(2),
    "p.data.copy_": lambda c: c.p.data.copy_(c.w),
    "p.data.clamp_": lambda c: c.p.data.clamp_(-0.1, 0.1),
    "BasicSR EMA line": _ema,
    "apply(init_fn) with w.data.normal_()": lambda c: c.m.apply(_init_fn),
    "p.data.mul_ under inference_mode": _inference_data_write,
    "Adam(fused=True).step": _step(lambda ps: torch.optim.Adam(ps, lr=0.1, fused=True)),      # torch's fused optimizer kernel: no .data in sight
    # ---- in place on the parameter (or a detached alias of it): the parameter's counter moves, the buffer's does not -----------------
    "no_grad p.mul_": _nograd(lambda c: c.p.mul_(2)),
    "p.detach().add_": lambda c: c.p.detach().add_(1),
    "p.detach().copy_": lambda c: c.p.detach().copy_(c.w),
    "nn.init.normal_": lambda c: nn.init.normal_(c.p),
    "_foreach_mul_": _nograd(lambda c: torch._foreach_mul_(list(c.m.parameters()), 0.5)),
    "Adam(foreach=True).step": _step(lambda ps: torch.optim.Adam(ps, lr=0.1, foreach=True)),
    "Adam(foreach=False).step": _step(lambda ps: torch.optim.Adam(ps, lr=0.1, foreach=False)),
    "SGD.step": _step(lambda ps: torch.optim.SGD(ps, lr=0.1)),
    "load_state_dict": lambda c: c.m.load_state_dict(c.other.state_dict()),
    "swa_utils.AveragedModel.update_parameters x2": _swa,
    # ---- on the buffer itself: its counter moves, the parameter's does not ----------------------------------------------------------------
    "flat.add_": lambda c: c.flat.add_(1),
    # ---- the parameter leaves the buffer: nothing in the buffer changes, the layout check of flatten_parameters has to notice -------------
    "vector_to_parameters": _vector,
    "p.data = tensor": _rebind,
    "to(float64).to(float32)": lambda c: c.m.to(torch.float64).to(torch.float32),
    "load_state_dict(assign=True)": lambda c: c.m.load_state_dict(copy.deepcopy(c.other.state_dict()), assign=True),
}
AVERAGED = {"swa_utils.AveragedModel.update_parameters x2"}

#                                                       flat_version p_version moved  same_param flat_changed
EXPECT = {
    "p.data.mul_":                                          (0, 0, False, True, True),
    "p.data.copy_":                                         (0, 0, False, True, True),
    "p.data.clamp_":                                        (0, 0, False, True, True),
    "BasicSR EMA line":                                     (0, 0, False, True, True),
    "apply(init_fn) with w.data.normal_()":                 (0, 0, False, True, True),
    "p.data.mul_ under inference_mode":                     (0, 0, False, True, True),
    "Adam(fused=True).step":                                (0, 0, False, True, True),      # the fused kernel bumps nothing either
    "no_grad p.mul_":                                       (0, 1, False, True, True),
    "p.detach().add_":                                      (0, 1, False, True, True),
    "p.detach().copy_":                                     (0, 1, False, True, True),
    "nn.init.normal_":                                      (0, 1, False, True, True),
    "_foreach_mul_":                                        (0, 1, False, True, True),
    "Adam(foreach=True).step":                              (0, 1, False, True, True),
    "Adam(foreach=False).step":                             (0, 1, False, True, True),
    "SGD.step":                                             (0, 1, False, True, True),
    "load_state_dict":                                      (0, 1, False, True, True),
    "swa_utils.AveragedModel.update_parameters x2":         (0, 2, False, True, True),
    "flat.add_":                                            (1, 0, False, True, True),
    "vector_to_parameters":                                 (0, 0, True, True, False),
    "p.data = tensor":                                      (0, 0, True, True, False),
    "to(float64).to(float32)":                              (0, 0, True, True, False),
    "load_state_dict(assign=True)":                         (0, None, True, False, False),
}


def observe(name):
    c = _Ctx(averaged=name in AVERAGED)
    m, flat, p = c.m, c.flat, c.p
    off = sum(q.numel() for q in m.a.parameters())
    assert p.data_ptr() == flat.data_ptr() + 4 * off and off > 0          # laid out, and not at the start
    fv, pv, ptr, before = flat._version, p._version, p.data_ptr(), flat.clone()
    WRITES[name](c)
    now = m.b.weight
    seen = (flat._version - fv, now._version - pv if now is p else None, now.data_ptr() != ptr, now is p, not torch.equal(flat, before))
    return seen, c


def test_every_idiom_has_its_row():
    assert list(WRITES) == list(EXPECT)


@pytest.mark.parametrize("name", list(WRITES))
def test_what_torch_does_to_a_flattened_parameter(name):
    seen, c = observe(name)
    print(f"{name}: flat_version +{seen[0]}, p_version {seen[1]}, moved {seen[2]}, same_param {seen[3]}, flat_changed {seen[4]}")
    assert seen == EXPECT[name]
    # what the module makes of it at its next forward: the layout check keeps the buffer where every parameter is still in place, and
    # lays a new one -- holding the parameters' present values -- where one left
    values = [q.detach().clone() for q in c.m.parameters()]
    again = c.m.flatten_parameters()
    assert (again is not c.flat) == seen[2]
    off = 0
    for q, v in zip(c.m.parameters(), values):
        assert q.data_ptr() == again.data_ptr() + 4 * off and torch.equal(q.detach(), v)
        assert torch.equal(again[off:off + q.numel()].view(q.shape), v)
        off += q.numel()


def test_the_version_sum_misses_exactly_the_data_writes_and_the_fused_optimizer():
    """_param_version moves for every write that leaves the parameters in place, except those through `.data` and the step of torch's
    fused Adam (one kernel over all parameters that bumps no counter): the reason no packed copy may be kept on its word"""
    blind = []
    for name in WRITES:
        c = _Ctx(averaged=name in AVERAGED)
        before = c.m._param_version()
        WRITES[name](c)
        c.m.flatten_parameters()
        if c.m._param_version() == before and c.m._flat is c.flat:
            blind.append(name)
    assert blind == [n for n in WRITES if EXPECT[n][:3] == (0, 0, False)] and len(blind) == 7


def test_parameters_built_under_inference_mode_have_no_version_counter():
    """... for good: after flatten_parameters pointed their .data at a normal tensor is_inference() answers False, and `_version` and
    autograd still refuse them.  _param_version refuses them by name instead of passing torch's message on, and flatten_parameters
    itself (all that a forward without a graph needs) works"""
    from xmm_superres_denoise.models.modules.flat_params import tracks_version
    with torch.inference_mode():
        m = _Tiny(0)
        m.load_state_dict(_Tiny(1).state_dict())
    assert all(p.is_inference() and not tracks_version(p) for p in m.parameters())
    flat = m.flatten_parameters()
    assert not flat.is_inference() and tracks_version(flat)
    assert not any(p.is_inference() or tracks_version(p) for p in m.parameters())
    assert m.b.weight.data_ptr() == flat.data_ptr() + 4 * 6
    with pytest.raises(RuntimeError, match="Inference tensors do not track version counter"):
        m.b.weight._version
    with pytest.raises(RuntimeError, match="Inference tensors do not track version counter"):
        nn.functional.linear(torch.zeros(1, 4), m.b.weight).sum().backward()
    with pytest.raises(RuntimeError, match="_Tiny: the parameters are inference tensors") as e:
        m._param_version()
    assert isinstance(e.value.__cause__, RuntimeError) and "version counter" in str(e.value.__cause__)
    with pytest.raises(RuntimeError, match="_Tiny: the parameters are inference tensors"):
        m._param_version()
    with torch.inference_mode():
        assert m.flatten_parameters() is flat
    assert all(tracks_version(p) for p in _Tiny(0).parameters())
