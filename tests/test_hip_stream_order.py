"""Stream order: every entry point enqueues ALL of its work -- kernels, hipMemsetAsync, device-to-device copies, the read-backs behind
a stream synchronize -- on the stream it is given (engine/engine.py: "the stateless entry points launch on the current stream";
ops.py: "run asynchronously on the current stream").  parallel.py's overlapped gradient exchange and every torch.cuda.stream user
depend on it; the kernel tests cannot see it, because they run on torch's default stream with the device idle before and after, where
a launch on stream 0 gives the same bits.

One helper, `late`, makes the property observable without any luck of timing.  For an entry fn(bufs) and two input sets of the same
shapes, `real` and `decoy` (other values; another magnitude where a max-|x| slot is involved):
  1. default stream: want = fn(real), twice, bit for bit equal (the reproducibility claim);
  2. default stream: fn(decoy), synchronize -- the plan of the shape is built, the workspaces hold the decoy's intermediates, the live
     input buffers hold the decoy; the host's enqueue time of fn is measured here, and once more on the idle side stream (where torch's
     allocator starts with an empty pool), the longer of the two counts;
  3. side stream (torch's pool streams are non-blocking: stream 0 does not wait for them): a delay, a copy of `real` into the live
     buffers, got = fn(live), an event `done`;
  4. vacuity guard: the delay's end event has not completed just before fn is called and, for an asynchronous entry, neither it nor
     `done` has completed when the host returns (the delay spun through the whole enqueue) -- a test whose delay ran out fails as
     "delay too short", it does not pass;
  5. synchronize, got == want bit for bit for every output.
Whatever fn puts on another stream, or reads through a path that does not wait for the side stream, runs while the delay is still
spinning: it sees the decoy (or the decoy's intermediates, or a slot the decoy left) and the outputs differ.

The delay is torch.cuda._sleep, calibrated once per module with an event pair (a chain of matmuls where _sleep does not spin); its
length is a multiple of the measured enqueue time plus a floor, capped well below a second.  test_zz_delay_report prints the
calibration and the longest delay.  Three streams in all: default, side, and the reader of test_hip_staged_grads.py."""
import json
import os
import time

import numpy as np
import pytest
import torch

import gen_common as gc
from oracle import oracle
from util_hip import G

pytestmark = pytest.mark.gpu

FLOOR_MS, MULT, CAP_MS = 25.0, 6.0, 600.0      # delay = min(CAP, max(FLOOR, MULT x the host's enqueue time of the entry))
CAL_CYCLES = 20_000_000
_S = {"side": None, "reader": None, "cyc_per_ms": None, "mm_ms": None, "mm": None, "rows": []}


def streams():
    """the module's two extra streams (side, reader): made once, shared by test_hip_staged_grads.py"""
    if _S["side"] is None:
        _S["side"], _S["reader"] = torch.cuda.Stream(), torch.cuda.Stream()
        for s in (_S["side"], _S["reader"]):      # a stream's first submission creates its queue: not behind a delay
            with torch.cuda.stream(s):
                torch.zeros(16, device="cuda")
        torch.cuda.synchronize()
    return _S["side"], _S["reader"]


def _calibrate():
    if _S["cyc_per_ms"] is not None or _S["mm_ms"] is not None:
        return
    side, _ = streams()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        torch.cuda._sleep(100_000)          # the stream's first submission (queue creation) is not part of the measurement
        a.record()
        torch.cuda._sleep(CAL_CYCLES)
        b.record()
    side.synchronize()
    ms = a.elapsed_time(b)
    if ms >= 1.0:
        _S["cyc_per_ms"] = CAL_CYCLES / ms
        return
    # _sleep does not spin on this device: a chain of large matmuls instead, timed the same way
    _S["mm"] = torch.randn(4096, 4096, device="cuda")
    with torch.cuda.stream(side):
        _S["mm"] @ _S["mm"]
        a.record()
        for _ in range(8):
            _S["mm"] @ _S["mm"]
        b.record()
    side.synchronize()
    _S["mm_ms"] = a.elapsed_time(b) / 8


def delay(ms):
    """enqueue about `ms` milliseconds of bounded spinning on the current stream"""
    _calibrate()
    if _S["cyc_per_ms"] is not None:
        torch.cuda._sleep(int(ms * _S["cyc_per_ms"]))
    else:
        for _ in range(int(ms / _S["mm_ms"]) + 1):
            _S["mm"] @ _S["mm"]


def same_bits(a, b):
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and a.device.type == b.device.type and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def late(fn, real, decoy, what, syncs=False, want=None):
    """The helper of the module docstring.  fn(bufs) -> tuple of output tensors, all of its work on the current stream; bufs are the
    live input buffers (fn may update them in place and return them: they are re-filled before every run).  `syncs`: the entry
    synchronizes its stream inside, so only the guard in front of the call applies.  `want`: outputs established elsewhere (the solo
    results of the in-flight tests) instead of step 1."""
    side, _ = streams()
    _calibrate()
    assert len(real) == len(decoy) and all(r.shape == d.shape and r.dtype == d.dtype for r, d in zip(real, decoy)), what
    assert any(not same_bits(r, d) for r, d in zip(real, decoy)), f"{what}: the decoy is the real input"
    live = [torch.empty_like(r) for r in real]

    def fill(src):
        for l, s in zip(live, src):
            l.copy_(s)
    torch.cuda.synchronize()
    if want is None:
        fill(real)
        want = [o.clone() for o in fn(live)]
        fill(real)
        again = [o.clone() for o in fn(live)]
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(want, again)):
            assert same_bits(a, b), f"{what}: output {i} of two runs on the default stream is not reproducible"
    host_ms = 0.0
    for stream in (torch.cuda.current_stream(), side):      # the decoy on the default stream, then once more on the idle side stream:
        fill(decoy)                                         # its first allocations there (torch's pools are per stream) are not part of
        torch.cuda.synchronize()                            # the timed enqueue behind the delay, and the longer of the two sizes the delay
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            fn(live)
            host_ms = max(host_ms, (time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    fill(decoy)
    torch.cuda.synchronize()
    ms = min(CAP_MS, max(FLOOR_MS, MULT * host_ms))
    end, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(side):
        delay(ms)
        end.record()
        for l, r in zip(live, real):
            l.copy_(r, non_blocking=True)
        spinning_before = not end.query()
        got = list(fn(live))
        done.record()
    # the delay's own end event is the stronger witness: while it is pending, nothing fn enqueued behind it has run (a `done` that is
    # merely not yet processed microseconds after its record would say nothing)
    pending_after = not done.query() and not end.query()
    side.synchronize()
    torch.cuda.synchronize()
    _S["rows"].append((what, host_ms, ms, spinning_before, pending_after, syncs))
    print(f"[late] {what}: enqueue {host_ms:.2f} ms, delay {ms:.1f} ms, delay still running before the call {spinning_before}, "
          f"delay still running when the host returned {pending_after}{' (entry synchronizes inside)' if syncs else ''}")
    assert spinning_before, f"{what}: delay too short: {ms:.1f} ms had run out before the entry was called"
    assert syncs or pending_after, f"{what}: delay too short: it had run out when the host returned (enqueue {host_ms:.2f} ms, delay {ms:.1f} ms)"
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"{what}: output {i} behind a late producer differs from the default-stream result"
    return got


def in_flight(fn, real_a, real_b, decoy, what):
    """Two calls behind ONE delay on the side stream, no host synchronization between them: each must give its solo result of the
    default stream (A alone, B alone, the device synchronized in between)."""
    k = len(real_a)
    solo = []
    for r in (real_a, real_b):
        torch.cuda.synchronize()
        solo += [o.clone() for o in fn([t.clone() for t in r])]
        torch.cuda.synchronize()
    return late(lambda b: tuple(fn(b[:k])) + tuple(fn(b[k:])), list(real_a) + list(real_b), list(decoy) + list(decoy), what, want=solo)


# ---------------------------------------------------------------------------------------------------------------
# the helper can fail: torch-only entries that misbehave in one way each
# ---------------------------------------------------------------------------------------------------------------
def _toy():
    real = [torch.arange(4096, dtype=torch.float32, device="cuda")]
    return real, [-real[0] - 1.0]


def test_helper_passes_an_entry_that_stays_on_its_stream():
    real, decoy = _toy()
    (got,) = late(lambda b: (b[0] * 2.0 + 1.0,), real, decoy, "toy: in order")
    assert torch.equal(got, real[0] * 2.0 + 1.0)


def test_helper_catches_one_op_on_the_default_stream():
    def bad(b):
        out = torch.empty_like(b[0])
        with torch.cuda.stream(torch.cuda.default_stream()):
            torch.mul(b[0], 2.0, out=out)
        return (out,)
    with pytest.raises(AssertionError, match="differs from the default-stream result"):
        late(bad, *_toy(), "toy: one op on stream 0")


def test_helper_catches_an_input_read_before_the_streams_turn():
    def bad(b):
        with torch.cuda.stream(torch.cuda.default_stream()):
            snap = b[0].clone()                 # the read does not wait for the producer
        return (snap * 2.0,)                    # the arithmetic is on the right stream
    with pytest.raises(AssertionError, match="differs from the default-stream result"):
        late(bad, *_toy(), "toy: early read")


def test_helper_catches_a_read_back_that_ignores_the_side_stream():
    out = torch.zeros(4096, device="cuda")

    def bad(b):
        torch.mul(b[0], 2.0, out=out)
        with torch.cuda.stream(torch.cuda.default_stream()):
            return (out.cpu(),)                 # a synchronous copy behind a synchronize of stream 0
    with pytest.raises(AssertionError, match="differs from the default-stream result"):
        late(bad, *_toy(), "toy: read-back through stream 0")


def test_helper_calls_a_delay_that_ran_out_too_short(monkeypatch):
    """no delay at all and an entry that waits for its own work: whichever guard sees it first, the verdict is "delay too short" """
    import sys
    monkeypatch.setattr(sys.modules[__name__], "FLOOR_MS", 0.0)
    monkeypatch.setattr(sys.modules[__name__], "MULT", 0.0)
    real, decoy = _toy()

    def slow(b):
        y = b[0] * 2.0
        torch.cuda.current_stream().synchronize()
        return (y,)
    with pytest.raises(AssertionError, match="delay too short"):
        late(slow, real, decoy, "toy: no delay")


# ---------------------------------------------------------------------------------------------------------------
# RRDB engine
# ---------------------------------------------------------------------------------------------------------------
# (kind, filters, math, image channels, num_upsample, x shape): the three math modes at the shipped width, a zero-padded width (8
# filters run as 32), two planes per tensor (64 filters) and the generic-width path (more than 8 image channels: exact fp32 kernels)
NETS = {"f16x3": ("dn", 32, "f16x3", 1, 1, (2, 1, 19, 22)), "bf16x6": ("dn", 32, "bf16x6", 1, 1, (2, 1, 19, 22)),
        "fp32": ("dn", 32, "fp32", 1, 1, (2, 1, 19, 22)), "padded8": ("dn", 8, "f16x3", 1, 1, (2, 1, 19, 22)),
        "wide64": ("dn", 64, "f16x3", 1, 1, (2, 1, 19, 22)), "generic9ch": ("dn", 8, "fp32", 9, 1, (1, 9, 19, 21))}
_NETS = {}


def flat_state(kind, nf, blocks, seed, ch=1, nup=1, gain=1.0):
    st = gc.make_state(kind, nf, blocks, seed, num_upsample=nup, gain=gain, last_bias=0.3 if kind == "sr" else None, in_ch=ch, out_ch=ch)
    return torch.from_numpy(oracle.flatten_state(st)).cuda()


def net(name):
    """-> (engine, packed with `flat`; flat; decoy parameters; real x; decoy x of another magnitude)"""
    if name not in _NETS:
        from xmm_superres_denoise.engine import Engine
        kind, nf, math, ch, nup, shape = NETS[name]
        eng = Engine(kind, ch, ch, nf, 1, nup)
        eng.set_math(math)
        flat, other = flat_state(kind, nf, 1, 7001, ch, nup), flat_state(kind, nf, 1, 7002, ch, nup, gain=0.5)
        x = torch.from_numpy(gc.make_input(shape, 7003)).cuda()
        xd = (37.0 * torch.from_numpy(gc.make_input(shape, 7004))).cuda()
        _NETS[name] = (eng, flat, other, x, xd)
    eng, flat, other, x, xd = _NETS[name]
    eng.pack(flat)
    return eng, flat, other, x, xd


def _dy_like(y, seed):
    return torch.from_numpy(gc.make_input(tuple(y.shape), seed) - 0.5).cuda()


@pytest.mark.parametrize("name", list(NETS))
def test_pack_with_the_parameters_written_late(name):
    eng, flat, other, x, _ = net(name)

    def fn(b):
        eng.pack(b[0])
        return (eng.forward(x),)
    late(fn, [flat], [other], f"rrdb {name}: pack")
    eng.pack(flat)


@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("name", list(NETS))
def test_forward(name, save):
    eng, _, _, x, xd = net(name)
    late(lambda b: (eng.forward(b[0], save_for_backward=save),), [x], [xd], f"rrdb {name}: forward save={save}")


def test_l1_loss():
    eng, _, _, x, xd = net("f16x3")
    y, yd = eng.forward(x), eng.forward(xd)
    t, td = _dy_like(y, 7011) + 0.5, 3.0 * _dy_like(y, 7012)
    late(lambda b: eng.l1_loss(b[0], b[1]), [y, t], [yd, td], "rrdb: l1_loss")


@pytest.mark.parametrize("name", list(NETS))
def test_backward(name):
    eng, _, _, x, xd = net(name)
    dy = _dy_like(eng.forward(x), 7021)

    def fn(b):
        eng.forward(b[0], save_for_backward=True)
        g = torch.full((eng.nparams,), float("nan"), device="cuda")
        dx = eng.backward(b[1], g, need_dx=True)
        return dx, g
    late(fn, [x, dy], [xd, 2.0 ** 9 * _dy_like(dy, 7022)], f"rrdb {name}: backward")


def test_adam_step_with_the_gradients_written_late():
    eng, flat, other, _, _ = net("f16x3")
    g = torch.Generator().manual_seed(7031)
    rnd = lambda s=1.0: (s * torch.randn(flat.numel(), generator=g)).cuda()      # noqa: E731
    real = [flat.clone(), rnd(1e-3), rnd(1e-4), rnd(1e-4).abs()]
    decoy = [other.clone(), rnd(1.0), rnd(1e-2), rnd(1e-2).abs()]

    def fn(b):
        eng.adam_step(b[0], b[1], b[2], b[3], step=3, lr=1e-3)
        return b[0], b[2], b[3]
    late(fn, real, decoy, "rrdb: adam_step")


@pytest.mark.parametrize("memory_efficient", [False, True])
def test_module_forward_then_autograd_backward(memory_efficient):
    """m(x) then y.backward(dy): autograd issues the backward on the forward's stream"""
    from xmm_superres_denoise.models import GeneratorRRDB_DN
    m = GeneratorRRDB_DN(1, 1, 32, 1, memory_efficient=memory_efficient)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in gc.make_state("dn", 32, 1, 7041).items()})
    m = m.cuda().set_math("f16x3")
    x = torch.from_numpy(gc.make_input((2, 1, 19, 22), 7042)).cuda()
    dy = _dy_like(x, 7043)

    def fn(b):
        for p in m.parameters():
            p.grad = None
        xg = b[0].detach().requires_grad_(True)
        y = m(xg)
        y.backward(b[1])
        return y.detach(), xg.grad, torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    late(fn, [x, dy], [41.0 * x.flip(3), 2.0 ** 8 * dy.flip(2)], f"rrdb module: forward + autograd backward, memory_efficient={memory_efficient}")


# ---------------------------------------------------------------------------------------------------------------
# the paper loss
# ---------------------------------------------------------------------------------------------------------------
def _paper_loss():
    from xmm_superres_denoise.utils import create_loss, load_loss_config
    return create_loss(*load_loss_config("linear"))      # 0.5 psnr + 0.5 ms_ssim: 304 pixels a side is the smallest image ms_ssim takes


def _loss_pairs():
    import make_golden_loss as mg
    return [[torch.from_numpy(a).cuda() for a in mg.loss_inputs(1, 304, 304, seed)] for seed in (7051, 7052)]


def _loss_fn(loss):
    def fn(b):
        tot, dy = loss.value_and_grad(b[0], b[1])
        return tot, dy, loss.last_values
    return fn


def test_paper_loss_value_and_grad():
    real, decoy = _loss_pairs()
    late(_loss_fn(_paper_loss()), real, [0.25 * decoy[0], 0.25 * decoy[1]], "paper loss: value_and_grad")


# ---------------------------------------------------------------------------------------------------------------
# the forward-only networks, from the smallest golden configuration of each
# ---------------------------------------------------------------------------------------------------------------
def _golden_net(family, case):
    import importlib
    gen, tst = importlib.import_module("gen_" + family), importlib.import_module("test_hip_" + family)
    z = np.load(os.path.join(G, f"{family}_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = tst._module(cfg, gen.make_state(cfg, int(z["seed"])))
    return m, torch.from_numpy(z["x"]).cuda()


@pytest.mark.parametrize("family,case,math", [("restormer", "d_ffn150", "fp32")] + [(f, c, m) for f, c in (("swinfir", "b_shifted_odd_w"), ("hat", "b_odd_sizes"),
                                                                                     ("swinir", "h_dn_imgrange255")) for m in ("fp32", "bf16x6")])
def test_forward_only_networks(family, case, math):
    """swinfir_b runs its FourierUnit (resi_connection "SFB"): the FFT passes and their twiddle table are in the forward"""
    m, x = _golden_net(family, case)
    m.set_math(math)

    def fn(b):
        with torch.no_grad():
            return (m(b[0]),)
    late(fn, [x], [(1.0 - x).flip(3) * 0.5], f"{family} {case} {math}: forward")


# ---------------------------------------------------------------------------------------------------------------
# ops.py: forward plus backward through autograd; one optimiser step of TrainableSwinIR
# ---------------------------------------------------------------------------------------------------------------
def _op_entry(op):
    """bufs = the op's differentiable inputs + the incoming gradient -> (y, every input gradient)"""
    def fn(b):
        ins = [t.detach().requires_grad_(True) for t in b[:-1]]
        y = op(*ins)
        y.backward(b[-1])
        return (y.detach(),) + tuple(t.grad for t in ins)
    return fn


def _other(ts, k=3.0):
    return [k * t.flip(0) + 0.125 for t in ts]


def test_ops_linear():
    from test_hip_sw_ops import _lin_inputs
    from xmm_superres_denoise import ops
    real = list(_lin_inputs(480, 10, 12, True))
    late(_op_entry(lambda a, w, b: ops.linear(a, w, b, act="gelu", chunk=112)), real, _other(real), "ops.linear 480 x 10 -> 12, gelu: forward + backward")


def test_ops_conv3x3():
    from test_hip_sw_ops import _conv_inputs
    from xmm_superres_denoise import ops
    real = list(_conv_inputs(2, 5, 7, 6, 6))
    late(_op_entry(lambda x, w, b: ops.conv3x3(x, w, b, act="lrelu", chunk=100)), real, _other(real), "ops.conv3x3 2 x 5 x 7, 6 -> 6, lrelu: forward + backward")


def test_ops_layer_norm():
    from test_hip_sw_kernels import _ln_params
    from xmm_superres_denoise import ops
    g = torch.Generator().manual_seed(7065)
    x = (torch.randn(7, 65, generator=g) * 3 + 0.7).cuda()
    w, b = _ln_params(65, g)
    real = [x, w, b, torch.randn(7, 65, generator=g).cuda()]
    late(_op_entry(ops.layer_norm), real, _other(real), "ops.layer_norm 7 x 65: forward + backward")


def test_ops_window_attention():
    from test_hip_sw_kernels import _attn_inputs
    from xmm_superres_denoise import ops
    B, H, W, C, heads, ws, shift = 1, 6, 9, 8, 2, 3, 1
    qkv, table, scale = _attn_inputs(B, H, W, C, heads, ws)
    real = [qkv, table, torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(7066)).cuda()]
    late(_op_entry(lambda q, t: ops.window_attention(q, t, H, W, heads, ws, shift, scale)), real, _other(real, 0.5),
         "ops.window_attention 6 x 9, window 3, shift 1: forward + backward")


@pytest.mark.parametrize("family", ["swinir", "swinfir"])
def test_trainable_swin_optimiser_step(family):
    """SwinIRTrainer.train_step (forward of the composed ops, l1, autograd backward, Adam) of TrainableSwinIR and TrainableSwinFIR at
    their smallest test configurations, from the same parameters and moments every run: they are inputs, restored on the current
    stream before the step.  The step is asynchronous: nothing in it may hold the host until the stream has drained (the wrappers once
    uploaded the module's mean from pageable host memory in every forward, which does)."""
    from xmm_superres_denoise.train import SwinIRTrainer
    if family == "swinir":
        import gen_swinir as gen
        from test_hip_swinir_train import DN as cfg, _build
        shape, tshape = (2, 1, 18, 21), (2, 1, 18, 21)
    else:
        import gen_swinfir as gen
        from test_hip_swinfir_train import A as cfg, _build
        shape, tshape = (2, 1, 8, 12), (2, 1, 16, 24)
    trainer = SwinIRTrainer(_build(cfg, 7071), lr=1e-3)
    params = trainer.params
    p0 = torch.cat([p.detach().reshape(-1) for p in params]).clone()
    x, xd = (torch.from_numpy(gen.make_input(shape, s)).cuda() for s in (7072, 7074))
    t, td = (torch.from_numpy(gen.make_input(tshape, s)).cuda() for s in (7073, 7075))

    def fn(b):
        with torch.no_grad():
            off = 0
            for p in params:
                p.copy_(b[2][off:off + p.numel()].view(p.shape))
                off += p.numel()
            trainer.m.copy_(b[3])
            trainer.v.copy_(b[4])
        trainer.step_count = 0
        loss = trainer.train_step(b[0], b[1])
        return loss, torch.cat([p.detach().reshape(-1) for p in params]), trainer.m, trainer.v
    zero = torch.zeros_like(p0)
    late(fn, [x, t, p0, zero, zero], [xd * 0.5, td, p0 * 0.75, zero + 1e-3, zero + 1e-6], f"Trainable{family}: one optimiser step")


# ---------------------------------------------------------------------------------------------------------------
# metrics: predictions and targets written late
# ---------------------------------------------------------------------------------------------------------------
def _photon(shape, seed):
    import ext_metrics_torch as E
    return [t.float().cuda() for t in E.photon_pair(shape, torch.Generator().manual_seed(seed))]


def test_ext_metrics_eval():
    from xmm_superres_denoise.engine import ExtMetricsEngine
    eng = ExtMetricsEngine()
    late(lambda b: (eng.eval(b[0], b[1]),), _photon((2, 61, 53), 7081), _photon((2, 61, 53), 7082), "ext metrics: eval 2 x 61 x 53")


def test_fsim_eval():
    from xmm_superres_denoise.engine import FsimEngine
    eng = FsimEngine()
    late(lambda b: (eng.eval(b[0], b[1]),), _photon((2, 61, 53), 7083), _photon((2, 61, 53), 7084), "fsim: eval 2 x 61 x 53")


# ---------------------------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------------------------
def test_compose_batch_with_the_pool_written_late():
    from test_hip_transform_kernels import make_planes, words
    from xmm_superres_denoise.engine import compose_batch
    Hin, Win, res = 5, 7, 8
    mask = torch.from_numpy((np.arange(Hin * Win).reshape(Hin, Win) % 5 != 0).astype(np.uint8)).cuda()

    def pool(seed):
        planes = make_planes(np.random.default_rng(seed), 4, 1, Hin, Win, True, seed)
        return torch.from_numpy(np.stack([words(p.reshape(-1), True) for p in planes])).cuda()
    late(lambda b: (compose_batch(b[0], [0, 2, 3], [1, -1, 0], [3, 1, -1], mask, Hin, Win, res, 0.0022336, "sqrt"),), [pool(7091)], [pool(7092)],
         "transforms: compose_batch 3 x 5 x 7 -> 8")


def test_mask_pad_normalize():
    from xmm_superres_denoise.engine import mask_pad_normalize
    g = torch.Generator().manual_seed(7093)
    counts, other = (torch.randint(0, 50, (2, 20, 13), generator=g, dtype=torch.int32).cuda() for _ in range(2))
    mask = (torch.rand(20, 13, generator=g) > 0.2).to(torch.uint8).cuda()
    late(lambda b: (mask_pad_normalize(b[0], mask, 16, 0.0022336, "asinh"),), [counts], [other + 7], "transforms: mask_pad_normalize 2 x 20 x 13 -> 16")


def test_normalize():
    from xmm_superres_denoise.engine import normalize
    g = torch.Generator().manual_seed(7094)
    img = (torch.rand(3, 1, 17, 23, generator=g) * 0.003).cuda()
    late(lambda b: (normalize(b[0], 0.0022336, "log"), normalize(b[0], 0.0022336, "sqrt", inverse=True)), [img], [img.flip(3) * 0.5], "transforms: normalize")


def test_image_upsample():
    from xmm_superres_denoise.engine import image_upsample
    x = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(7095)).cuda()
    late(lambda b: (image_upsample(b[0], 3),), [x], [-x.flip(2)], "transforms: image_upsample x3")


# ---------------------------------------------------------------------------------------------------------------
# two calls in flight behind one delay: A's input is 2^12 times B's
# ---------------------------------------------------------------------------------------------------------------
def test_two_forwards_in_flight_start_from_clean_max_slots():
    """f16x3 zeroes the max-|x| slots of the plan with a hipMemsetAsync on the call's stream: B behind A must not inherit A's maxima"""
    eng, _, _, x, xd = net("f16x3")
    in_flight(lambda b: (eng.forward(b[0]),), [2.0 ** 12 * x], [x], [xd], "in flight: two forwards, f16x3")


@pytest.mark.parametrize("name", ["f16x3", "bf16x6"])
def test_two_train_passes_in_flight(name):
    """forward + l1_loss + backward twice: the slots of the backward plan, the weight-gradient partial buffers and the loss's
    double partials are reset / rewritten in stream order"""
    eng, _, _, x, xd = net(name)
    t = _dy_like(x, 7101) + 0.5

    def fn(b):
        y = eng.forward(b[0], save_for_backward=True)
        loss, dy = eng.l1_loss(y, b[1])
        g = torch.full((eng.nparams,), float("nan"), device="cuda")
        dx = eng.backward(dy * b[2], g, need_dx=True)      # b[2]: one number, the scale of the incoming gradient
        return y, loss, dx, g
    one = torch.ones(1, device="cuda")
    in_flight(fn, [2.0 ** 12 * x, 2.0 ** 12 * t, 2.0 ** 12 * one], [x, t, one], [xd, t.flip(3), 3.0 * one], f"in flight: two train passes, {name}")


def test_two_paper_losses_in_flight():
    (p, t), (pd, td) = _loss_pairs()
    in_flight(_loss_fn(_paper_loss()), [2.0 ** 12 * p, 2.0 ** 12 * t], [p, t], [0.25 * pd, 0.25 * td], "in flight: two paper losses")


def test_zz_delay_report():
    """what the log records: the calibration, the longest delay, and per call that the delay was still running"""
    rows = _S["rows"]
    assert rows, "no call of the helper ran in this session"
    how = f"torch.cuda._sleep at {_S['cyc_per_ms']:.0f} cycles per ms" if _S["cyc_per_ms"] else f"a matmul chain at {_S['mm_ms']:.3f} ms per 4096^3 product"
    print(f"[delay] {how}; {len(rows)} calls; longest delay {max(r[2] for r in rows):.1f} ms; longest enqueue {max(r[1] for r in rows):.2f} ms")
    assert max(r[2] for r in rows) <= CAP_MS
