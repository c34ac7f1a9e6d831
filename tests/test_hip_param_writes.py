"""The seam between torch and the engines: every way torch code rewrites parameters (tests/test_param_writes_host.py pins what torch
itself does for each), through every engine-backed module, and the training-side contract of the modules that train.

A module's parameters are views into one flat buffer; an engine keeps a packed copy of some of them and reads the others as stored,
through the pointer of the last pack.  After a write W on a module that has already run a forward, its next forward must be bit for
bit the forward of a freshly constructed module that loaded the written module's state dict, must lie within the family's float64 bar
on that state dict, and must differ from the forward before W by far more than the bar (100 x).  Every W changes at least one
parameter the engine packs and one it reads as stored, which rules out the half-stale state:

  family                          packed (C pack function)                                   read as stored
  GeneratorRRDB_DN / _SR          rrdb.0.RDB3.conv5.weight  (xsd_pack_weights: every conv    rrdb.0.RDB3.conv5.bias  (conv_launch: p.bias =
                                  weight into MFMA panels)                                   params + bias_off)
  Restormer                       refinement.0.attn.project_out.weight  (xsd_restormer_      refinement.0.norm1.body.weight  (only the pw1s
                                  pack_weights: the pointwise convs, transposed into wt)     are transposed; the rest: r->params + offset)
  SwinFIR / HAT / SwinIR          layers.0.residual_group.blocks.1.attn.qkv.weight           layers.0.residual_group.blocks.0.norm1.weight;
  (and the Trainable wrappers,    (sw_kernels.h pack_weights: every Lin of r->lins)          HAT: ...blocks.0.conv_block.cab.3.attention.3.bias
  which pack nothing)                                                                        (PP(r, off): params + off)

The bars are the families' own: RRDB 2e-5 absolute (test_hip_network._widths_vs_float64), Restormer 1e-4 (test_hip_restormer), SwinFIR /
HAT / SwinIR 1e-5 in fp32 (their repack tests), bf16x6 and the Trainable wrappers within twice the error of the same restatement run in
fp32 (test_hip_swinir, test_hip_sw_kernels._assert_within_2x_of_fp32; the wrappers with a non-zero yardstick).  The float64 yardsticks
are oracle.torch_forward and tests/golden/*_torch.py.

Between forward and backward (GeneratorRRDB_*): a write through `.data` is invisible to torch, so neither torch's saved-tensor check
nor the recompute guard can object.  The plain backward runs on the activations and the packed weights of the forward: its gradients
are bit for bit those without the write.  The memory_efficient backward packs and re-runs the forward: its gradients are bit for bit
those of a module that held the new weights all along (for the dy of the old forward).  Pinned here, not changed.

Figures of one run on an MI355X (profiles/r31_param_write_tests.log; the file takes about 20 s, the slowest case 2.9 s: the first
use of the bf16x6 kernels): worst max |y - float64| over all writes 2.1e-7 / 1.7e-7 (RRDB DN / SR, bar 2e-5), 4.6e-7 (Restormer, 1e-4), 6.7e-7 /
5.4e-7 / 4.1e-7 (SwinFIR / HAT / SwinIR, 1e-5); worst error relative to the fp32 restatement's 1.06 (SwinIR bf16x6), 0.82 / 0.37 (the
wrappers; bar 2); the least any write moves an output is 326 bars (Restormer).  On the parent commit the file fails the 25 cases
(forward-only family, write through .data or fused Adam) and the 9 inference-mode constructions, and passes the rest
(profiles/r31_mutants.log)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import parameters_to_vector, vector_to_parameters
from torch.optim.swa_utils import AveragedModel

import gen_common as gc
import gen_hat as gh
import gen_restormer as gr
import gen_swinfir as gs
import gen_swinir as gi
import hat_torch as ht
import restormer_torch as rt
import swinfir_torch as st
import swinir_torch as sit
from oracle import oracle
from test_hip_hat import SMALL as HAT_SMALL
from test_hip_network import ADAM_SOLID
from test_hip_sw_kernels import _assert_within_2x_of_fp32
from test_hip_swinfir_train import A as SWINFIR_TRAIN

pytestmark = pytest.mark.gpu

# ADAM_SOLID (test_hip_network, set on the DN net with tools/calib_adam.py) asks that 0.6 of the parameters keep a gradient above 1e-5 of the
# largest one through the three steps, where the oracle's own gradients give 0.6485.  The same count on the SR net, from the oracle
# alone (DESIGN.md section 32 has the table by floor and by layer group): 0.3520, because the floor is relative to the largest gradient,
# which the convs behind the pixel shuffle set, and only 27 % of the dense blocks' weights stay above it.  The SR bar keeps DN's
# margin under the oracle's value: 0.6 / 0.6485 of 0.3520.
ADAM_SOLID_SR_SHARE = ADAM_SOLID[1] * 0.3520 / 0.6485

QKV = "layers.0.residual_group.blocks.1.attn.qkv.weight"
NORM1 = "layers.0.residual_group.blocks.0.norm1.weight"


# ---- the families -------------------------------------------------------------------------------------------------------------------
class Family:
    math = None
    trainable = False

    def build(self, sd=None, seed=0, **kw):
        """a new module of the family on the device, with the generator's state of `seed` or the state dict `sd`"""
        m = self.construct(**kw)
        if sd is None:
            sd = {k: torch.from_numpy(np.array(v)) for k, v in self.state(seed).items()}
        m.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
        m = m.cuda()
        if self.math:
            self.core(m).set_math(self.math)
        return m

    def core(self, m):
        return m

    def input(self, seed=1):
        return torch.from_numpy(gc.make_input(self.shape, seed)).cuda()

    def out_shape(self):
        B, C, H, W = self.shape
        return (B, C, H * self.scale, W * self.scale)

    def within_bar(self, y, sd, x, what):
        """asserts the family's float64 bar; returns (how far an output has moved, in the bar's measure) -> multiples of the bar"""
        y64 = self.restate({k: v.detach().double() if v.is_floating_point() else v.detach() for k, v in sd.items()}, x.double())
        if self.tol is not None:
            err = float((y.double() - y64).abs().max())
            print(f"{what}: max |y - float64| {err:.3e} (bar {self.tol:.0e})")
            assert err < self.tol, (what, err)
            return lambda a, b: float((a - b).abs().max()) / self.tol
        y32 = self.restate({k: v.detach().clone() for k, v in sd.items()}, x)
        rms32 = _assert_within_2x_of_fp32(y, y32, y64, what)
        if self.trainable:
            assert rms32 > 0, (what, "the fp32 yardstick is exact here")
        return lambda a, b: float((a - b).pow(2).mean().sqrt()) / (2 * rms32 + 1e-30)


class RRDB(Family):
    tol = 2e-5
    shape = (1, 1, 16, 24)

    def __init__(self, kind):
        self.kind, self.scale = kind, 2 if kind == "sr" else 1
        self.packed, self.stored = "rrdb.0.RDB3.conv5.weight", "rrdb.0.RDB3.conv5.bias"

    def state(self, seed):
        return gc.make_state(self.kind, 32, 1, 700 + seed, num_upsample=1, last_bias=0.3 if self.kind == "sr" else None)

    def construct(self, memory_efficient=False):
        from xmm_superres_denoise.models import GeneratorRRDB_DN, GeneratorRRDB_SR
        if self.kind == "dn":
            return GeneratorRRDB_DN(1, 1, 32, 1, memory_efficient=memory_efficient)
        return GeneratorRRDB_SR(1, 1, 32, 1, num_upsample=1, memory_efficient=memory_efficient)

    def restate(self, sd, x):
        return oracle.torch_forward(self.kind, 32, 1, {k: v.cpu() for k, v in sd.items()}, x.cpu(), num_upsample=1).to(x.device)


class Transformer(Family):
    tol = 1e-5
    packed, stored = QKV, NORM1

    def __init__(self, cls, gen, restate, cfg, shape, scale, math="fp32", tol=1e-5, packed=None, stored=None):
        self.cls, self.gen, self._restate, self.cfg, self.shape, self.scale, self.math, self.tol = cls, gen, restate, cfg, shape, scale, math, tol
        self.packed, self.stored = packed or QKV, stored or NORM1

    def state(self, seed):
        return self.gen.make_state(self.cfg, 800 + seed)

    def construct(self):
        import xmm_superres_denoise.models as M
        return getattr(M, self.cls)(**self.gen.full_cfg(**self.cfg))

    def restate(self, sd, x):
        cfg = self.gen.full_cfg(**self.cfg) if self.cls == "Restormer" else self.cfg
        return self._restate(sd, x, **cfg)


class Trainable(Transformer):
    trainable = True

    def __init__(self, wrapper, *a, **kw):
        super().__init__(*a, **kw)
        self.wrapper, self.math, self.tol = wrapper, None, None

    def construct(self):
        import xmm_superres_denoise.models as M
        return getattr(M, self.wrapper)(super().construct(), drop_path_rate=0.0)

    def core(self, m):
        return m.module


SWINIR_CFG = gi.CASES["a_dn_reflect"]["cfg"]
assert next(iter(gi.CASES)) == "a_dn_reflect" and next(iter(gs.CASES)) == "a_clamped_window" and next(iter(gr.CASES)) == "a_dim8_default"
FAMILIES = OrderedDict([
    ("rrdb_dn", RRDB("dn")),
    ("rrdb_sr", RRDB("sr")),
    ("restormer", Transformer("Restormer", gr, rt.restormer_forward, gr.CASES["a_dim8_default"]["cfg"], (1, 3, 16, 24), 1, tol=1e-4,
                              packed="refinement.0.attn.project_out.weight", stored="refinement.0.norm1.body.weight")),
    ("swinfir", Transformer("SwinFIR", gs, st.swinfir_forward, gs.CASES["a_clamped_window"]["cfg"], (1, 1, 13, 13), 2)),
    ("hat", Transformer("HAT", gh, ht.hat_forward, HAT_SMALL, (1, 1, 16, 24), 2,
                        stored="layers.0.residual_group.blocks.0.conv_block.cab.3.attention.3.bias")),
    ("swinir", Transformer("SwinIR", gi, sit.swinir_forward, SWINIR_CFG, (1, 1, 16, 24), 1)),
    ("swinir_bf16x6", Transformer("SwinIR", gi, sit.swinir_forward, SWINIR_CFG, (1, 1, 16, 24), 1, math="bf16x6", tol=None)),
    ("trainable_swinir", Trainable("TrainableSwinIR", "SwinIR", gi, sit.swinir_forward, SWINIR_CFG, (1, 1, 16, 24), 1)),
    ("trainable_swinfir", Trainable("TrainableSwinFIR", "SwinFIR", gs, st.swinfir_forward, SWINFIR_TRAIN, (1, 1, 8, 12), 2)),
])
FORWARD_ONLY = ("restormer", "swinfir", "hat", "swinir", "swinir_bf16x6")
TRAINING = ("rrdb_dn", "rrdb_sr", "trainable_swinir", "trainable_swinfir")


# ---- the writes -----------------------------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, fam, m):
        self.fam, self.m, self.core = fam, m, fam.core(m)
        self._other = None
        self.run = m                      # the module whose forward is looked at after the write (the averaged copy, for swa_utils)

    @property
    def P(self):
        return dict(self.core.named_parameters())[self.fam.packed]

    @property
    def S(self):
        return dict(self.core.named_parameters())[self.fam.stored]

    @property
    def other(self):
        """a second module of the family with other weights (the EMA's source, the state dict to load), built when a write asks for it"""
        if self._other is None:
            self._other = self.fam.build(seed=1)
        return self._other

    def other_sd(self):
        return {k: v.detach().clone() for k, v in self.other.state_dict().items()}


def _hand_grads(c):
    for i, p in enumerate(c.core.parameters()):
        p.grad = torch.sin(torch.arange(p.numel(), device=p.device, dtype=torch.float32) + i).view(p.shape)


def _opt_step(make):
    def write(c):
        _hand_grads(c)
        make(list(c.core.parameters())).step()
        for p in c.core.parameters():
            p.grad = None
    return write


def _data_mul_copy(c):
    c.P.data.mul_(0.5)
    c.S.data.copy_(c.S.data + 2.0)


def _ema(c, decay=0.5):                   # BasicSR: the EMA network is the one that validates
    for ema_p, p in zip(c.core.parameters(), c.fam.core(c.other).parameters()):
        ema_p.data.mul_(decay).add_(p.data, alpha=1 - decay)
    c.S.data.add_(2.0)


def _detach_copy(c):
    c.P.detach().copy_(c.P.detach() * 0.5)
    c.S.detach().copy_(c.S.detach() + 2.0)


def _init_normal(c):
    nn.init.normal_(c.P, std=0.05)
    nn.init.normal_(c.S, mean=2.0, std=0.5)


def _apply_init(c):
    P, S = c.P, c.S

    def init_fn(mod):
        for p in mod.parameters(recurse=False):
            if p is P:
                p.data.normal_(0.0, 0.05)
            elif p is S:
                p.data.normal_(2.0, 0.5)
    c.m.apply(init_fn)


def _foreach(c):
    with torch.no_grad():
        torch._foreach_mul_(list(c.core.parameters()), 0.5)
        c.S.add_(2.0)


def _load_strict(c):
    c.m.load_state_dict(c.other_sd())
    with torch.no_grad():
        c.S.add_(2.0)


def _load_assign(c):
    c.m.load_state_dict(c.other_sd(), assign=True)
    with torch.no_grad():
        c.S.add_(2.0)


def _vector(c):
    vector_to_parameters(0.5 * parameters_to_vector(c.core.parameters()), c.core.parameters())
    c.S.data.add_(2.0)


def _rebind_one(c):
    c.P.data = (c.P.data * 0.5).clone()   # this parameter alone leaves the buffer: the layout splits in the middle
    c.S.data.add_(2.0)


def _flat_write(c):
    flat = c.core.flat_parameters()
    flat.mul_(0.5)
    off = 0
    for k, p in c.core.named_parameters():
        if k == c.fam.stored:
            flat[off:off + p.numel()].add_(2.0)
        off += p.numel()


def _cpu_edit_cuda(c):
    c.m.cpu()
    with torch.no_grad():
        c.P.mul_(0.5)
        c.S.add_(2.0)
    c.m.cuda()


def _swa(c):
    avg = AveragedModel(c.m)
    avg.update_parameters(c.m)            # copies
    with torch.no_grad():
        c.P.mul_(-1.0)
        c.S.add_(4.0)
    avg.update_parameters(c.m)            # averages: P -> 0, S -> + 2
    c.run = avg.module


def _inference_data(c):
    with torch.inference_mode():
        c.P.data.mul_(0.5)
        c.S.data.add_(2.0)


WRITES = OrderedDict([
    ("1 p.data.mul_ / p.data.copy_", _data_mul_copy),
    ("2 BasicSR EMA line", _ema),
    ("3 p.detach().copy_", _detach_copy),
    ("4a nn.init.normal_(p)", _init_normal),
    ("4b apply(init_fn) with w.data.normal_()", _apply_init),
    ("5 _foreach_mul_", _foreach),
    ("6a Adam(foreach=True) step", _opt_step(lambda ps: torch.optim.Adam(ps, lr=0.05, foreach=True))),
    ("6b Adam(fused=True) step", _opt_step(lambda ps: torch.optim.Adam(ps, lr=0.05, fused=True))),
    ("6c SGD step", _opt_step(lambda ps: torch.optim.SGD(ps, lr=0.05))),
    ("7a load_state_dict", _load_strict),
    ("7b load_state_dict(assign=True)", _load_assign),
    ("8 vector_to_parameters", _vector),
    ("9 p.data = tensor", _rebind_one),
    ("10 write to flat_parameters()", _flat_write),
    ("11 cpu(), edit, cuda()", _cpu_edit_cuda),
    ("12 swa_utils.AveragedModel", _swa),
    ("13 p.data write under inference_mode", _inference_data),
])


@pytest.mark.parametrize("write", list(WRITES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_forward_after_a_write_is_a_fresh_modules_forward(family, write):
    fam = FAMILIES[family]
    m = fam.build().eval()
    x = fam.input()
    with torch.no_grad():
        before = m(x).clone()
        c = Ctx(fam, m)
        p_old, s_old = c.P.detach().clone(), c.S.detach().clone()
        WRITES[write](c)
        run = c.run
        sd = {k: v.detach().clone() for k, v in run.state_dict().items()}
        assert not torch.equal(sd[fam.packed], p_old) and not torch.equal(sd[fam.stored], s_old)      # a packed one and a stored one
        after = run(x)
        assert after.shape == fam.out_shape() and torch.isfinite(after).all()
        fresh = fam.build(sd=sd).eval()
        want = fresh(x)
        same = torch.equal(after, want)
        print(f"{family} / {write}: max |after - fresh| {float((after - want).abs().max()):.3e}, max |after - before| {float((after - before).abs().max()):.3e}")
        assert same, "the forward after the write is not the forward of a fresh module with the written state"
        moved = fam.within_bar(after, sd, x, f"{family} / {write}")(after, before)
        print(f"{family} / {write}: the output moved by {moved:.3g} bars")
        assert moved > 100, moved
        assert torch.equal(run(x), after)                                                             # and stays


# ---- modules built under inference mode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_module_built_under_inference_mode_runs_and_refuses_training_by_name(family):
    fam = FAMILIES[family]
    x = fam.input()
    with torch.no_grad():
        want = fam.build()(x)
    with torch.inference_mode():
        m = fam.build()
        y = m(x)
        again = m(x)
    assert torch.equal(y, want) and torch.equal(again, want)
    with torch.no_grad():
        assert torch.equal(m(x), want)                          # outside the mode, without a graph: works too
    name = type(m).__name__
    if not fam.trainable and family not in ("rrdb_dn", "rrdb_sr"):
        # a forward-only family in grad mode, outside the mode (a model loaded under inference_mode and called without no_grad): the
        # forward works and hands out a graph node, and the backward refuses in the family's usual words
        out = m(x)
        assert torch.equal(out.detach(), want) and out.requires_grad
        with pytest.raises(RuntimeError, match="training is not on the MI355X engine"):
            out.sum().backward()
        return
    # a family that trains: its parameters can never be trained (no version counter, autograd cannot save them), and the training-mode
    # forward says so naming inference tensors and the module, not in torch's words
    with pytest.raises(RuntimeError, match=f"{name}: .*inference tensors") as e:
        m.train()(x.clone().requires_grad_(True))
    print(f"{family}: {e.value}")
    assert "do not track version counter" not in str(e.value) and "cannot be saved for backward" not in str(e.value)
    with torch.no_grad():
        assert torch.equal(m.eval()(x), want)                   # and the refusal left the module usable


# ---- the training side ---------------------------------------------------------------------------------------------------------------
def _pass(net, x, dy, zero=True):
    """one forward / backward; returns (y, dx, {name: grad clone or None})"""
    if zero:
        for p in net.parameters():
            p.grad = None
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    y.backward(dy)
    return y.detach().clone(), xi.grad.clone(), OrderedDict((k, None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters())


def _dy(fam, seed):
    return torch.randn(fam.out_shape(), generator=torch.Generator().manual_seed(seed)).cuda()


def _name(fam, k):
    return ("module." + k) if fam.trainable else k


@pytest.mark.parametrize("family", TRAINING)
def test_frozen_subset(family):
    """one packed and one stored parameter frozen: their .grad stays None, every other gradient and dx are bit for bit the all-trainable
    run's, and so is the output"""
    fam = FAMILIES[family]
    net = fam.build().train()
    x, dy = fam.input(), _dy(fam, 5)
    y0, dx0, g0 = _pass(net, x, dy)
    assert all(g is not None for g in g0.values())
    frozen = {_name(fam, fam.packed), _name(fam, fam.stored)}
    for k, p in net.named_parameters():
        p.requires_grad_(k not in frozen)
    y1, dx1, g1 = _pass(net, x, dy)
    assert set(g1) == set(g0) and frozen <= set(g1)
    if not fam.trainable:      # what the generators' backward hands to autograd, which would drop a gradient nobody wants without a word
        from xmm_superres_denoise.models.modules.generator_rrdb import _split_flat
        outs = _split_flat(torch.zeros_like(net._flat), net._plist)
        assert [o is None for o in outs] == [not p.requires_grad for p in net._plist] and sum(o is None for o in outs) == 2
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    for k in g0:
        if k in frozen:
            assert g1[k] is None, k
        else:
            assert g1[k] is not None and torch.equal(g1[k], g0[k]), k
    for p in net.parameters():
        p.requires_grad_(True)
    y2, dx2, g2 = _pass(net, x, dy)                           # and thawed again: the first run
    assert torch.equal(dx2, dx0) and all(torch.equal(g2[k], g0[k]) for k in g0)


@pytest.mark.parametrize("family", TRAINING)
def test_gradient_accumulation(family):
    """two forward / backward passes on different inputs without zero_grad: p.grad is bit for bit g1 + g2 (summed by torch in fp32) of the
    two passes run apart; the same after zero_grad(set_to_none=False)"""
    fam = FAMILIES[family]
    net = fam.build().train()
    xa, xb, dya, dyb = fam.input(2), fam.input(3), _dy(fam, 6), _dy(fam, 7)
    _, _, ga = _pass(net, xa, dya)
    _, _, gb = _pass(net, xb, dyb)
    assert any(not torch.equal(ga[k], gb[k]) for k in ga)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    for how in ("grad is None", "zero_grad(set_to_none=False)"):
        if how == "grad is None":
            opt.zero_grad(set_to_none=True)
        else:
            opt.zero_grad(set_to_none=False)
            assert all(p.grad is not None and not p.grad.any() for p in net.parameters())
        _pass(net, xa, dya, zero=False)
        _, _, g = _pass(net, xb, dyb, zero=False)
        for k in ga:
            assert torch.equal(g[k], ga[k] + gb[k]), (how, k)


def _three_steps(fam, how, sd, x, t, lr):
    net = fam.build(sd=sd).train()
    if how == "project":
        if fam.trainable:
            from xmm_superres_denoise.train import SwinIRTrainer
            tr = SwinIRTrainer(net, lr=lr, betas=(0.9, 0.999))
        else:
            from xmm_superres_denoise.parallel import DataParallelTrainer
            tr = DataParallelTrainer(net, lr=lr)
        losses = [float(tr.train_step(x, t)) for _ in range(3)]
    else:
        opt = torch.optim.Adam(net.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8, foreach=how == "foreach")
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = F.l1_loss(net(x), t)
            loss.backward()
            opt.step()
            losses.append(float(loss))
    return torch.cat([p.detach().reshape(-1) for p in fam.core(net).parameters()]).double().cpu(), losses


_TRAJECTORY = {}


def _trajectory(family):
    """the float64 yardstick of three L1 + Adam steps, computed once per family and left unchanged"""
    if family in _TRAJECTORY:
        return _TRAJECTORY[family]
    fam = FAMILIES[family]
    C, H, W = (fam.shape[1], fam.shape[2], fam.shape[3]) if fam.trainable else (1, 24, 40)      # the generators: the shape ADAM_SOLID was set at
    x = torch.from_numpy(gc.make_input((2, C, H, W), 78)).cuda()
    t = torch.from_numpy(gc.make_input((2, C, H * fam.scale, W * fam.scale), 79)).cuda()
    out = dict(x=x, t=t)
    if fam.trainable:
        out["lr"] = 1e-3
        first = fam.build(seed=3)
        sd0 = out["sd"] = {k: v.detach().clone() for k, v in first.state_dict().items()}
        names = {k for k, _ in fam.core(first).named_parameters()}
        for dtype in (torch.float64, torch.float32):
            sd = OrderedDict((k, v.detach().to(dtype, copy=True).requires_grad_(True) if k in names else v.detach()) for k, v in sd0.items())
            params = [v for v in sd.values() if v.requires_grad]
            opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
            for _ in range(3):
                opt.zero_grad()
                F.l1_loss(fam.restate(sd, x.to(dtype)), t.to(dtype)).backward()
                opt.step()
            out[dtype] = torch.cat([p.detach().reshape(-1).double() for p in params]).cpu()
    else:
        out["lr"] = 1e-4
        state = gc.make_state(fam.kind, 32, 1, 77, num_upsample=1, last_bias=0.3 if fam.kind == "sr" else None)
        out["sd"] = {k: torch.from_numpy(v.copy()) for k, v in state.items()}
        p = oracle.flatten_state(state).copy()
        mo, vo = np.zeros_like(p), np.zeros_like(p)
        g_min = None
        for step in range(1, 4):
            _, _, _, go = oracle.l1_train(fam.kind, 32, 1, p, x.cpu().numpy(), t.cpu().numpy())
            g_min = np.abs(go) if g_min is None else np.minimum(g_min, np.abs(go))
            oracle.adam(p, go, mo, vo, step)
        out.update(start=oracle.flatten_state(state).astype(np.float64), end=p.astype(np.float64), solid=g_min > ADAM_SOLID[0] * np.abs(go).max())
    _TRAJECTORY[family] = out
    return out


@pytest.mark.parametrize("how", ["foreach", "single tensor", "project"])
@pytest.mark.parametrize("family", TRAINING)
def test_three_adam_steps_each_way_follow_the_float64_trajectory(family, how):
    """torch.optim.Adam(foreach=True), Adam(foreach=False) and what the project trains with (parallel.DataParallelTrainer: the engine's
    fused Adam on the flat buffer; train.SwinIRTrainer: torch's Adam over flat moment buffers).  torch documents none of its
    implementations as the same arithmetic as another, so none is held to another bit for bit: each is held to the float64
    trajectory by the family's own bar -- test_hip_network.test_train_step_adam_matches_oracle's for the generators (the accumulated
    update of every parameter whose gradient stays above ADAM_SOLID's floor within 5e-8 of the oracle's, nobody further than the three
    steps allow), test_five_adam_steps_follow_the_float64_trajectory's for the wrappers (rms distance at most twice torch fp32's)."""
    fam = FAMILIES[family]
    tj = _trajectory(family)
    mine, losses = _three_steps(fam, how, tj["sd"], tj["x"], tj["t"], tj["lr"])
    print(f"{family} / {how}: losses {losses}")
    if fam.trainable:
        rms = float((mine - tj[torch.float64]).pow(2).mean().sqrt())
        rms32 = float((tj[torch.float32] - tj[torch.float64]).pow(2).mean().sqrt())
        print(f"{family} / {how}: parameters after 3 Adam steps: rms {rms:.3e} | fp32 torch rms {rms32:.3e} (ratio {rms / rms32:.3f})")
        assert rms32 > 0 and rms <= 2 * rms32, (rms, rms32)
    else:
        d_eng, d_ora, solid = mine.numpy() - tj["start"], tj["end"] - tj["start"], tj["solid"]
        worst = float(np.abs(d_eng[solid] - d_ora[solid]).max())
        print(f"{family} / {how}: solid share {solid.mean():.3f}, max |update - oracle's| on them {worst:.3e}, anywhere {np.abs(d_eng - d_ora).max():.3e}")
        assert solid.mean() > (ADAM_SOLID[1] if fam.kind == "dn" else ADAM_SOLID_SR_SHARE)
        assert worst < 5e-8
        assert np.abs(d_eng - d_ora).max() < 2.5e-4
        assert np.median(np.abs(d_ora[solid])) > 1e-4


@pytest.mark.parametrize("memory_efficient", [False, True], ids=["plain", "memory_efficient"])
@pytest.mark.parametrize("family", ["rrdb_dn", "rrdb_sr"])
def test_data_write_between_forward_and_backward(family, memory_efficient):
    """see the module docstring: documented behaviour, pinned; no error is raised in either mode"""
    fam = FAMILIES[family]
    x, dy = fam.input(), _dy(fam, 8)
    net = fam.build(memory_efficient=memory_efficient).train()
    y0, dx0, g0 = _pass(net, x, dy)                           # no write
    for p in net.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    c = Ctx(fam, net)
    c.P.data.mul_(0.5)
    c.S.data.add_(2.0)
    y.backward(dy)
    g = OrderedDict((k, p.grad.detach().clone()) for k, p in net.named_parameters())
    assert torch.equal(y.detach(), y0)
    new = fam.build(sd=net.state_dict(), memory_efficient=memory_efficient).train()
    y1, dx1, g1 = _pass(new, x, dy)                           # the new weights all along
    assert not torch.equal(y1, y0) and not torch.equal(dx1, dx0)
    want_dx, want = (dx1, g1) if memory_efficient else (dx0, g0)
    assert torch.equal(xi.grad, want_dx)
    for k in g:
        assert torch.equal(g[k], want[k]), k
