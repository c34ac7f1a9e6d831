"""A backward stage's gradient range is final when the stage returns: everything that writes grads[off : off + cnt] of
xsd_grad_range(stage) is enqueued on the caller's stream by then, and no later stage touches the range again.  parallel.py hands the
range to RCCL (reduced in place, on RCCL's stream) or, under gloo, to a copy stream behind an event, while the later stages are
already being enqueued -- it is right only if both hold.

The test is parallel.py's gloo branch plus a poison that stands in for RCCL's in-place reduction: on a side stream behind a delay
(test_hip_stream_order.py: the helper's delay, streams and guards), forward + loss, then per stage, with no host synchronization
anywhere in the loop: backward_stage, an event, and on the reader stream behind that event a copy of the range into `snap` and NaN
over the range in the gradient vector.  Both vectors start as NaN.  After ONE synchronize: the ranges tile [0, nparams) exactly, snap
is the monolithic backward's gradient of the default stream bit for bit, and the gradient vector is poison throughout.  A decoy pass
on other data (other magnitude) in front leaves its intermediates in the workspace and its values in the live inputs, so a stage
that enqueued a writer elsewhere, or a range that a later stage rewrites, cannot come out equal.

The same through backward_recompute's last_chunk_hook with three tiles in chunks of two; the reference there is the same call run
synchronously on the default stream (the same arithmetic, so bit for bit)."""
import time

import pytest
import torch

import gen_common as gc
from test_hip_stream_order import CAP_MS, FLOOR_MS, MULT, delay, flat_state, same_bits, streams

pytestmark = pytest.mark.gpu
NAN = float("nan")

# (kind, filters, blocks, math, image channels, num_upsample, x shape)
NETS = {"dn32-f16x3": ("dn", 32, 2, "f16x3", 1, 1, (2, 1, 19, 22)), "dn32-bf16x6": ("dn", 32, 2, "bf16x6", 1, 1, (2, 1, 19, 22)),
        "dn32-fp32": ("dn", 32, 2, "fp32", 1, 1, (2, 1, 19, 22)), "sr32-up2": ("sr", 32, 2, "f16x3", 1, 2, (2, 1, 19, 22)),
        "padded16": ("dn", 16, 2, "f16x3", 1, 1, (2, 1, 19, 22)),          # nf_pad: the stage's pad-gather writes the caller's range
        "generic9ch": ("dn", 8, 1, "fp32", 9, 1, (1, 9, 19, 21))}          # more than 8 image channels: generic->grad_range


def _engine(name):
    from xmm_superres_denoise.engine import Engine
    kind, nf, blocks, math, ch, nup, shape = NETS[name]
    eng = Engine(kind, ch, ch, nf, blocks, nup)
    eng.set_math(math)
    flat = flat_state(kind, nf, blocks, 8001, ch, nup)
    eng.pack(flat)
    s = 2 ** nup if kind == "sr" else 1
    tshape = (shape[0], ch, shape[2] * s, shape[3] * s)
    x, xd = (torch.from_numpy(gc.make_input(shape, k)).cuda() for k in (8002, 8003))
    t, td = (torch.from_numpy(gc.make_input(tshape, k)).cuda() for k in (8004, 8005))
    return eng, flat, x, t, 29.0 * xd, td


def _nan(n):
    return torch.full((n,), NAN, device="cuda")


def _hand_over(reader, cur, g, snap, off, cnt):
    """parallel.py's gloo branch (an event behind the stage, the copy on another stream behind the event) + the poison"""
    ready = torch.cuda.Event()
    ready.record(cur)
    with torch.cuda.stream(reader):
        reader.wait_event(ready)
        snap[off:off + cnt].copy_(g[off:off + cnt], non_blocking=True)
        g[off:off + cnt].fill_(NAN)
    return ready


def _guards(what, spinning, pending, host_ms, ms):
    print(f"[staged] {what}: enqueue {host_ms:.2f} ms, delay {ms:.1f} ms, delay still running before the first call {spinning}, "
          f"delay still running and the last stage's event pending when the loop returned {pending}")
    assert spinning, f"{what}: delay too short: {ms:.1f} ms had run out before the forward was called"
    assert pending, f"{what}: delay too short: it had run out when the loop returned (enqueue {host_ms:.2f} ms, delay {ms:.1f} ms)"


@pytest.mark.parametrize("name", list(NETS))
def test_a_stages_range_is_final_when_the_stage_returns(name):
    eng, flat, x, t, xd, td = _engine(name)
    side, reader = streams()
    n = eng.nparams
    ranges = [eng.grad_range(st) for st in range(eng.num_stages)]
    pos = 0
    for off, cnt in sorted(ranges):         # pairwise disjoint, and together exactly [0, nparams)
        assert off == pos and cnt > 0, (name, ranges)
        pos += cnt
    assert pos == n, (name, ranges)
    # the reference: one monolithic backward on the default stream
    y1 = eng.forward(x, save_for_backward=True)
    loss1, dy1 = eng.l1_loss(y1, t)
    g1 = _nan(n)
    eng.backward(dy1, g1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g1).all())
    xl, tl, g2, snap = xd.clone(), td.clone(), _nan(n), _nan(n)

    def staged(scale):
        """forward + loss + the staged backward with its hand-overs, on the current stream, no host synchronization"""
        y = eng.forward(xl, save_for_backward=True)
        loss, dy = eng.l1_loss(y, tl)
        if scale != 1.0:
            dy = dy * scale
        for st, (off, cnt) in enumerate(ranges):
            eng.backward_stage(st, dy, g2)
            last = _hand_over(reader, torch.cuda.current_stream(), g2, snap, off, cnt)
        return y, loss, dy, last
    # the decoy pass: other data, a gradient 2^9 times larger, on the default stream and once more on the idle side stream (its first
    # allocations there are not part of the enqueue behind the delay); the longer enqueue sizes the delay
    host_ms = 0.0
    for stream in (torch.cuda.current_stream(), side):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            staged(2.0 ** 9)
            host_ms = max(host_ms, (time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    ms = min(CAP_MS, max(FLOOR_MS, MULT * host_ms))
    g2.fill_(NAN)
    snap.fill_(NAN)
    torch.cuda.synchronize()
    end = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay(ms)
        end.record()
        xl.copy_(x, non_blocking=True)
        tl.copy_(t, non_blocking=True)
        spinning = not end.query()
        y2, loss2, dy2, last = staged(1.0)
    pending = not last.query() and not end.query()      # the delay spun through the whole loop
    torch.cuda.synchronize()
    _guards(f"{name}: {eng.num_stages} stages", spinning, pending, host_ms, ms)
    assert same_bits(y2, y1) and same_bits(loss2, loss1) and same_bits(dy2, dy1), name
    bad = [st for st, (off, cnt) in enumerate(ranges) if not same_bits(snap[off:off + cnt], g1[off:off + cnt])]
    assert not bad, f"{name}: the ranges of stages {bad} were not final when their stage returned"
    assert bool(torch.isnan(g2).all()), f"{name}: a later stage wrote {int((~torch.isnan(g2)).sum())} elements of a range already handed over"


def test_recomputed_backward_hands_over_final_ranges_in_its_hook():
    from xmm_superres_denoise.models.modules.generator_rrdb import backward_recompute
    eng, flat, _, _, _, _ = _engine("dn32-f16x3")
    side, reader = streams()
    n = eng.nparams
    x, xd = (torch.from_numpy(gc.make_input((3, 1, 19, 22), k)).cuda() for k in (8011, 8012))
    dy, dyd = (torch.from_numpy(gc.make_input((3, 1, 19, 22), k) - 0.5).cuda() for k in (8013, 8014))
    ref = _nan(n)
    backward_recompute(eng, x, dy, ref, False, chunk=2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all())
    xl, dyl = (29.0 * xd).clone(), (2.0 ** 9 * dyd).clone()
    grads, snap = _nan(n), _nan(n)
    events = []

    def hook(st):
        off, cnt = eng.grad_range(st)
        events.append(_hand_over(reader, torch.cuda.current_stream(), grads, snap, off, cnt))
    host_ms = 0.0
    for stream in (torch.cuda.current_stream(), side):      # the decoy, as in the test above
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t0 = time.perf_counter()
            backward_recompute(eng, xl, dyl, grads, False, chunk=2, last_chunk_hook=hook)
            host_ms = max(host_ms, (time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    ms = min(CAP_MS, max(FLOOR_MS, MULT * host_ms))
    grads.fill_(NAN)
    snap.fill_(NAN)
    del events[:]
    torch.cuda.synchronize()
    end = torch.cuda.Event()
    with torch.cuda.stream(side):
        delay(ms)
        end.record()
        xl.copy_(x, non_blocking=True)
        dyl.copy_(dy, non_blocking=True)
        spinning = not end.query()
        backward_recompute(eng, xl, dyl, grads, False, chunk=2, last_chunk_hook=hook)
    pending = not events[-1].query() and not end.query()
    torch.cuda.synchronize()
    _guards("recompute, 3 tiles in chunks of 2", spinning, pending, host_ms, ms)
    assert len(events) == eng.num_stages
    assert same_bits(snap, ref), "a range was not final when last_chunk_hook was called for its stage"
    assert bool(torch.isnan(grads).all()), "a later stage wrote a range already handed over"
