"""What the library HOLDS on the device: every allocation of libxsd_hip.so goes through one ledger (csrc/xsd_ledger.h, csrc/xsd_mem.h),
read here through xsd_test_mem_stats and steered through xsd_test_mem_refuse (include/xsd.h).  No tolerance anywhere: every comparison
is an exact integer or a bit-for-bit equality.

  a. create, use (small shape, growth, small shape again, one refused call), destroy: live blocks and bytes are back at the baseline
  b. no product entry allocates in steady state; test entries that own temporaries free exactly what they allocate
  c. the fsim plan cache holds exactly the XSD_FSIM_PLANS most recently used sizes
  d. simulated refusals, swept over every allocation of every create and every growth path: XSD_ERR_NOMEM, nothing leaked, the handle
     usable afterwards with bit-identical results
  e. the Python side: modules that are dropped, copied, pickled, reloaded; training steps in steady state

Other modules' fixtures keep handles alive, so every test compares DELTAS inside a window that starts after gc.collect() and keeps the
collector off; foreign_frees must not move in any of them.  The refusal is simulated on the host (the n-th allocation answers
hipErrorOutOfMemory without reaching the runtime): no test approaches a real out-of-memory."""
import contextlib
import copy
import ctypes
import gc
import os
import pickle
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import gen_hat as gh
import gen_restormer as gr
import gen_swinfir as gs
import gen_swinir as gi

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_NOMEM = 0, -1, -2, -3, -4      # include/xsd.h
NAMES = ("live_blocks", "live_bytes", "allocs", "frees", "foreign_frees", "refused")
SENTINEL = 0x5EED5EED
FSIM_PLANS, FSIM_NF = 4, 16      # include/xsd.h: XSD_FSIM_PLANS; csrc/fsim.hip: 4 orientations x 4 scales of filters per plan


def _L():
    from xmm_superres_denoise.engine import _lib
    return _lib.load()


def stats():
    buf = (ctypes.c_int64 * 6)()
    assert _L().xsd_test_mem_stats(buf, 6) == OK
    return dict(zip(NAMES, (int(v) for v in buf)))


def live(s=None):
    s = s or stats()
    return s["live_blocks"], s["live_bytes"]


def moved(s):
    return s["allocs"], s["frees"]


@contextlib.contextmanager
def window():
    """the measured window: baseline after a collection, the collector off, the arm off before and after; foreign_frees stays"""
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    _L().xsd_test_mem_refuse(0)
    s0 = stats()
    try:
        yield s0
    finally:
        _L().xsd_test_mem_refuse(0)
        gc.enable()
    assert stats()["foreign_frees"] == s0["foreign_frees"]


def drop(e):
    """destroy the handle now (the wrappers' __del__ is their only destroy; it clears the handle, so a later collection does nothing)"""
    torch.cuda.synchronize()
    e.__del__()
    assert not getattr(e, "h", None)


_INPUTS = {}


def rand(shape, seed=0):
    key = (tuple(shape), seed)
    if key not in _INPUTS:
        _INPUTS[key] = torch.rand(shape, generator=torch.Generator().manual_seed(1000 + seed)).cuda()
    return _INPUTS[key]


def code_of(excinfo) -> int:
    m = re.search(r"libxsd_hip error (-?\d+):", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1))


# ---- the families: fresh() -> a packed engine wrapper, run(e, shape) -> its result as one tensor, bad(e) -> the code of a refused call ----
class Fam:
    def __init__(self, fresh, run, small, large, bad, train=None):
        self.fresh, self.run, self.small, self.large, self.bad, self.train = fresh, run, small, large, bad, train


def _rrdb(kind, cin, cout, nf, nup, math, small=(1, 16, 16), large=(2, 24, 40), blocks=1):
    from xmm_superres_denoise.engine import Engine
    held = {}

    def fresh():
        e = Engine(kind, cin, cout, nf, blocks, nup)
        if "p" not in held:
            held["p"] = (torch.randn(e.nparams, generator=torch.Generator().manual_seed(7)) * 0.05).cuda()
        e.set_math(math)
        e.pack(held["p"])
        return e

    def run(e, shape):
        return e.forward(rand((shape[0], cin, shape[1], shape[2])))

    def train(e, shape):
        x = rand((shape[0], cin, shape[1], shape[2]))
        y = e.forward(x, save_for_backward=True)
        dy = rand(tuple(y.shape), 1) - 0.5
        grads = torch.empty(e.nparams, device="cuda")
        dx = e.backward(dy, grads, need_dx=True)
        return torch.cat([y.reshape(-1), grads, dx.reshape(-1)])

    def bad(e):
        return e.L.xsd_forward(e.h, None, None, 1, 16, 16, 0, None)
    return Fam(fresh, run, small, large, bad, train)


def _module_fam(make_module, math, small, large, entry):
    held = {}

    def fresh():
        if "m" not in held:
            torch.manual_seed(11)
            held["m"] = make_module().cuda()
            held["flat"] = held["m"].flatten_parameters().detach()
        e = held["m"]._make_engine()
        e.set_math(math)
        e.pack(held["flat"])
        return e

    def run(e, shape):
        return e.forward(rand(shape))

    def bad(e):
        return getattr(e.L, entry)(e.h, None, None, 1, 8, 8, None)
    return Fam(fresh, run, small, large, bad)


SWINFIR = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=4, mlp_ratio=2.0, upscale=2,
               upsampler="pixelshuffle")                                 # resi_connection "SFB" (the default): the FourierUnit and its twiddles
SWINFIR_1CONV = dict(SWINFIR, resi_connection="1conv", drop_path_rate=0.0)      # test_hip_swinfir_train.py's net A
SWINIR_DN = dict(img_size=64, patch_size=1, in_chans=1, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=4, upscale=1, upsampler="",
                 drop_path_rate=0.0)                                     # test_hip_swinir_train.py's denoiser
HAT_A = dict(gh.CASES["a_shifted_ocab"]["cfg"])
RESTORMER = dict(inp_channels=1, out_channels=1, dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=[1, 2, 4, 8])


def _restormer(math="fp32"):
    from xmm_superres_denoise.models import Restormer
    return _module_fam(lambda: Restormer(**gr.full_cfg(**RESTORMER)), math, (1, 1, 8, 8), (2, 1, 16, 24), "xsd_restormer_forward")


def _swinfir(math):
    from xmm_superres_denoise.models import SwinFIR
    return _module_fam(lambda: SwinFIR(**gs.full_cfg(**SWINFIR)), math, (1, 1, 8, 12), (2, 1, 12, 16), "xsd_swinfir_forward")


def _hat(math):
    from xmm_superres_denoise.models import HAT
    return _module_fam(lambda: HAT(**gh.full_cfg(**HAT_A)), math, (1, 1, 16, 16), (1, 1, 16, 24), "xsd_hat_forward")


def _swinir(math):
    from xmm_superres_denoise.models import SwinIR
    return _module_fam(lambda: SwinIR(**gi.full_cfg(**SWINIR_DN)), math, (1, 1, 8, 12), (2, 1, 18, 21), "xsd_swinir_forward")


def _loss():
    from xmm_superres_denoise.utils.loss_functions import Loss

    def run(e, shape):
        out, dy = e._eval(rand(shape), rand(shape, 1), True)
        return torch.cat([out, dy.reshape(-1)])
    return Fam(lambda: Loss({"l1": 1.0, "psnr": 0.5, "ssim": 0.5}), run, (1, 24, 40), (2, 32, 48),
               lambda e: e.L.xsd_loss_eval(e.h, None, None, None, None, 1, 24, 40, None))


def _extm():
    from xmm_superres_denoise.engine.engine import ExtMetricsEngine
    return Fam(ExtMetricsEngine, lambda e, shape: e.eval(rand(shape), rand(shape, 1)), (1, 41, 41), (2, 64, 48),
               lambda e: e.L.xsd_ext_metrics_eval(e.h, None, None, None, 1, 41, 41, None))


def _fsim():
    from xmm_superres_denoise.engine.engine import FsimEngine
    return Fam(FsimEngine, lambda e, shape: e.eval(rand(shape), rand(shape, 1)), (1, 16, 16), (2, 20, 24),
               lambda e: e.L.xsd_fsim_eval(e.h, None, None, None, 1, 1, 16, 16, None))


FAMS = {
    "rrdb nf32 fp32": lambda: _rrdb("dn", 1, 1, 32, 0, "fp32"),
    "rrdb nf32 bf16x6": lambda: _rrdb("dn", 1, 1, 32, 0, "bf16x6"),
    "rrdb nf32 f16x3": lambda: _rrdb("dn", 1, 1, 32, 0, "f16x3"),
    "rrdb nf8 f16x3": lambda: _rrdb("dn", 1, 1, 8, 0, "f16x3"),
    "rrdb sr nf32 up1 f16x3": lambda: _rrdb("sr", 1, 1, 32, 1, "f16x3"),
    "rrdb nf48 padded f16x3": lambda: _rrdb("dn", 1, 1, 48, 0, "f16x3"),
    "rrdb generic width": lambda: _rrdb("dn", 9, 9, 8, 0, "fp32", small=(1, 9, 11), large=(2, 12, 16)),
    "loss": _loss,
    "ext metrics": _extm,
    "fsim": _fsim,
    "restormer": _restormer,
    "swinfir fp32": lambda: _swinfir("fp32"),
    "swinfir bf16x6": lambda: _swinfir("bf16x6"),
    "hat fp32": lambda: _hat("fp32"),
    "hat bf16x6": lambda: _hat("bf16x6"),
    "swinir fp32": lambda: _swinir("fp32"),
    "swinir bf16x6": lambda: _swinir("bf16x6"),
}
RRDB_TRAIN = [k for k in FAMS if k.startswith("rrdb")]


# ---- a. create, use, destroy returns everything ---------------------------------------------------------------------------
def _use_and_destroy(fam, s0, extra=None, run=None):
    run = run or fam.run
    e = fam.fresh()
    if extra:
        extra(e)
    r1 = run(e, fam.small)
    run(e, fam.large)
    r3 = run(e, fam.small)
    assert fam.bad(e) == ERR_ARG and _L().xsd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(r1, r3)                                  # the small shape after the growth: its first result bit for bit
    held = stats()
    assert held["live_blocks"] > s0["live_blocks"] and held["live_bytes"] > s0["live_bytes"]      # the ledger sees the handle
    drop(e)
    assert live() == live(s0)
    assert stats()["allocs"] - s0["allocs"] == stats()["frees"] - s0["frees"] > 0


@pytest.mark.parametrize("name", list(FAMS))
def test_create_use_destroy_returns_everything(name):
    fam = FAMS[name]()
    with window() as s0:
        _use_and_destroy(fam, s0)


@pytest.mark.parametrize("name", RRDB_TRAIN)
def test_create_train_destroy_returns_everything(name):
    fam = FAMS[name]()
    with window() as s0:
        _use_and_destroy(fam, s0, run=fam.train)


def test_destroy_with_debug_stamps_left_enabled_returns_everything():
    """xsd_debug_stamps(e, 1) allocates the stamp buffer; a handle destroyed with the stamps still on must give it back"""
    fam = FAMS["rrdb nf32 f16x3"]()
    with window() as s0:
        _use_and_destroy(fam, s0, extra=lambda e: _assert_ok(e.L.xsd_debug_stamps(e.h, 1, None)), run=fam.train)


def test_destroy_with_the_profile_left_enabled_returns_everything():
    fam = FAMS["rrdb nf32 f16x3"]()
    with window() as s0:
        _use_and_destroy(fam, s0, extra=lambda e: e.profile_enable(True), run=fam.train)


def _assert_ok(rc):
    assert rc == OK, _L().xsd_last_error()


# ---- b. steady state --------------------------------------------------------------------------------------------------------
def _assert_steady(call):
    """after two identical calls the third moves neither allocs nor frees"""
    call()
    call()
    torch.cuda.synchronize()
    s = stats()
    call()
    torch.cuda.synchronize()
    assert moved(stats()) == moved(s) and live() == live(s)


@pytest.mark.parametrize("name", list(FAMS))
def test_no_allocation_in_steady_state_forward(name):
    """xsd_forward / xsd_loss_eval / xsd_ext_metrics_eval / xsd_fsim_eval and the four transformer forwards in both math modes"""
    fam = FAMS[name]()
    with window():
        e = fam.fresh()
        _assert_steady(lambda: fam.run(e, fam.small))
        drop(e)


@pytest.mark.parametrize("name", RRDB_TRAIN)
def test_no_allocation_in_a_steady_training_step(name):
    """xsd_pack_weights, xsd_forward (saving), xsd_backward, then the same through xsd_backward_stage, xsd_adam_step, xsd_l1_loss"""
    fam = FAMS[name]()
    with window():
        e = fam.fresh()
        p = (torch.randn(e.nparams, generator=torch.Generator().manual_seed(3)) * 0.05).cuda()
        m, v, grads = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
        shape = fam.small
        cin = 9 if "generic" in name else 1
        x = rand((shape[0], cin, shape[1], shape[2]))

        def step():
            e.pack(p)
            y = e.forward(x, save_for_backward=True)
            loss, dy = e.l1_loss(y, rand(tuple(y.shape), 2))
            e.backward(dy, grads, need_dx=True)
            y = e.forward(x, save_for_backward=True)
            dx = torch.empty_like(x)
            for st in range(e.num_stages):
                e.backward_stage(st, dy, grads, dx=dx)
            e.adam_step(p, grads, m, v, 1)
        _assert_steady(step)
        drop(e)


def test_compose_batch_allocates_nothing():
    from xmm_superres_denoise.engine.engine import compose_batch
    pool = torch.randint(0, 100, (4, 35), dtype=torch.int32, generator=torch.Generator().manual_seed(5)).cuda()
    with window():
        _assert_steady(lambda: compose_batch(pool, [0, 3, 1], [1, -1, 2], None, None, 7, 5, 9, None, big_endian=False))


@pytest.mark.parametrize("net", ["swinir", "swinfir"])
def test_the_twelve_sw_op_entries_never_allocate(net, monkeypatch):
    """"no allocation, no synchronisation".  Every call of every xsd_sw_op_* entry during two training steps of the
    tiny trainable Swin nets is watched: none moves a ledger counter, and each net's steps reach all twelve entries."""
    from xmm_superres_denoise.engine import _lib
    from xmm_superres_denoise.models import SwinFIR, SwinIR, TrainableSwinFIR, TrainableSwinIR
    L = _L()
    names = [n for n in _lib.ENTRIES if n.startswith("xsd_sw_op_")]
    assert len(names) == 12
    seen, offenders = set(), []
    for n in names:
        def spy(*a, _real=getattr(L, n), _n=n):
            before = stats()
            rc = _real(*a)
            if moved(stats()) != moved(before):
                offenders.append(_n)
            seen.add(_n)
            return rc
        monkeypatch.setattr(L, n, spy)
    torch.manual_seed(13)
    if net == "swinir":
        m, x = TrainableSwinIR(SwinIR(**gi.full_cfg(**SWINIR_DN)).cuda()).train(), rand((2, 1, 18, 21))
    else:
        m, x = TrainableSwinFIR(SwinFIR(**gs.full_cfg(**SWINFIR_1CONV)).cuda()).train(), rand((2, 1, 8, 12))
    with window():
        for _ in range(2):
            y = m(x.clone().requires_grad_(True))
            y.square().mean().backward()
        torch.cuda.synchronize()
        del y
    assert not offenders, sorted(set(offenders))
    # both nets run 3x3 convs, linears, LayerNorms and window attention forward and backward, each backward with its scratch query
    assert seen == set(names), sorted(set(names) - seen)


def _temporaries():
    from xmm_superres_denoise.engine import engine as E
    g = torch.Generator().manual_seed(17)
    a, w, b = torch.randn(37, 20, generator=g).cuda(), torch.randn(9, 20, generator=g).cuda(), torch.randn(9, generator=g).cuda()
    xi, wi = torch.randn(1, 5, 7, 6, generator=g).cuda(), torch.randn(8, 6, 3, 3, generator=g).cuda()
    xt, tt = torch.randn(2, 35, 12, generator=g).cuda(), torch.randn(2, 35, 12, generator=g).cuda()
    w1, b1, w2, b2 = (torch.randn(s, generator=g).cuda() for s in ((3, 12), (3,), (12, 3), (12,)))
    img = torch.rand(1, 2, 9, 10, generator=g).cuda()
    rq, rt, rw, rx = (torch.randn(s, generator=g).cuda() for s in ((1, 24, 48), (2,), (8, 8), (1, 8, 48)))
    va, vw, vy = torch.randn(6, 4, generator=g).cuda(), torch.randn(8, 4, generator=g).cuda(), torch.zeros(6, 8, device="cuda")
    # entry -> (call, device allocations it owns per call: read off csrc/sw_gemm_s3x.h test_gemm, csrc/hat.hip, csrc/swinir.hip)
    return {
        "xsd_sw_test_gemm fp32": (lambda: E.sw_gemm(a, w, b), 1),
        "xsd_sw_test_gemm bf16x6": (lambda: E.sw_gemm(a, w, b, math="bf16x6"), 1),
        "xsd_sw_test_gemm conv3": (lambda: E.sw_conv3x3(xi, wi), 1),
        "xsd_swinir_test_nearest_conv": (lambda: E.swinir_nearest_conv(xi, wi), 1),
        "xsd_hat_test_channel_mean": (lambda: E.hat_channel_mean(xt), 1),
        "xsd_hat_test_ca_combine": (lambda: E.hat_ca_combine(xt.clone(), tt, w1, b1, w2, b2, 0.5), 2),
        "xsd_swinir_test_pad with a mean": (lambda: E.swinir_pad(img, 4, mean=[0.2, 0.4]), 1),
        "xsd_swinir_test_pad without": (lambda: E.swinir_pad(img, 4), 0),
        "xsd_loss_test_scale": (lambda: _loss_scale(), 1),                                   # csrc/loss_kernels.hip loss_test_scale: its workspace
        # the DevMem users (csrc/xsd_test_entries.hip): pack_single owns the two panels and the descriptor, in f16x3 also the two fp32
        # panels the fp16 images are split from; edge_pack_one owns the four weight forms in one buffer
        "xsd_test_conv3x3 fp32": (lambda: _conv_entry("fp32", "fwd"), 3),
        "xsd_test_conv3x3 f16x3": (lambda: _conv_entry("f16x3", "fwd"), 5),
        "xsd_test_conv3x3_bwd fp32": (lambda: _conv_entry("fp32", "bwd"), 3),
        "xsd_test_conv3x3_bwd f16x3": (lambda: _conv_entry("f16x3", "bwd"), 5),
        "xsd_test_conv3x3_ex bf16x6": (lambda: _conv_entry("bf16x6", "ex"), 3),
        "xsd_test_conv3x3_ex f16x3": (lambda: _conv_entry("f16x3", "ex"), 5),
        "xsd_test_edge_expand": (lambda: _edge_entry("expand"), 1),
        "xsd_test_edge_reduce": (lambda: _edge_entry("reduce"), 1),
        # the Scratch users (csrc/restormer.hip): the transposed weight; the attention hooks add the per-image matrix and the Gram
        # partial sums, the wide one its attention rows as well
        "xsd_restormer_test_pw": (lambda: E.restormer_pw(rq[:, :8], rw), 1),
        "xsd_restormer_test_attention": (lambda: E.restormer_channel_attention(rq, rt, rw, None, rx.clone(), 2), 3),
        "xsd_restormer_test_attention_wide": (lambda: E.restormer_channel_attention_wide(rq, rt, rw, None, rx.clone(), 2), 4),
        # test_gemm_view (csrc/sw_gemm_s3x.h): the packed weight, in the instance SwinFIR / HAT run and in SwinIR's
        "xsd_sw_test_gemm_view": (lambda: E.sw_gemm_view(va, vw, vy, conv3=False, B=1, H=1, W=6, cin=4, N=8, lda=4, ldy=8), 1),
        "xsd_swinir_test_gemm_view": (lambda: E.sw_gemm_view(va, vw, vy, conv3=False, B=1, H=1, W=6, cin=4, N=8, lda=4, ldy=8, ext=True), 1),
        # a PRODUCT entry that allocates per call (csrc/mfma_stream_probe.hip: the staged image, the sink, the clock pairs), a
        # measurement that blocks for `seconds`: Engine.probe_mfma_stream, which bench.py calls once per run, outside its timed steps
        "xsd_probe_mfma_stream": (lambda: _conv_engine("fp32").probe_mfma_stream("f16", 0.01), 3),
        # a GenericNet of one conv per call (xsd_test_gconv): whatever it allocates, it frees
        "xsd_test_gconv": (lambda: _gconv_entry(), None),
    }


def _loss_scale():
    from test_hip_loss_kernels import run_scale
    run_scale(_L(), rand((1, 24, 40)).cpu().numpy(), rand((1, 24, 40), 1).cpu().numpy())


_CONV_ENGINES = {}


def _conv_engine(math):
    if math not in _CONV_ENGINES:
        _CONV_ENGINES[math] = FAMS["rrdb nf32 " + math]().fresh()
    return _CONV_ENGINES[math]


def _conv_entry(math, which):
    """one 32 -> 32 conv on planes [1][8][32][32] through xsd_test_conv3x3, its backward or the _ex form with a plain epilogue"""
    from util_hip import ptr_array
    from xmm_superres_denoise.engine import _lib
    e = _conv_engine(math)
    x, out = [rand((1, 8, 32, 32)) - 0.5], [torch.empty(1, 8, 32, 32, device="cuda")]
    w, b = (rand((32, 32, 3, 3), 3) - 0.5) / 17, rand((32,), 4)
    if which == "fwd":
        rc = e.L.xsd_test_conv3x3(e.h, ptr_array(x), 1, w.data_ptr(), b.data_ptr(), ptr_array(out), 1, 0.2, 1, 8, 32, None)
    elif which == "bwd":
        g, dw, db = rand((1, 8, 32, 32), 5) - 0.5, torch.empty_like(w), torch.empty(32, device="cuda")
        rc = e.L.xsd_test_conv3x3_bwd(e.h, ptr_array(x), 1, w.data_ptr(), g.data_ptr(), ptr_array(out), dw.data_ptr(), db.data_ptr(), 1, 8, 32, None)
    else:
        d = (_lib.XsdTestOut * 1)()
        ctypes.memset(d, 0, ctypes.sizeof(d))
        d[0].p, d[0].a1, d[0].a2, d[0].slope, d[0].mslope = out[0].data_ptr(), 1.0, 1.0, 0.2, 1.0
        rc = e.L.xsd_test_conv3x3_ex(e.h, ptr_array(x), 1, 0, w.data_ptr(), b.data_ptr(), d, 1, 0, None, 1, 8, 32, None)
    _assert_ok(rc)


def _edge_entry(which):
    """test_hip_edge_kernels.py's own callers of the two edge hooks (guard bands and all), on the fp32 engine"""
    import numpy as np
    import test_hip_edge_kernels as K
    e, rng = _conv_engine("fp32"), np.random.default_rng(23)
    if which == "expand":
        K.run_expand(e, rng.random((1, 1, 9, 13), dtype=np.float32), 0, K.make_w_first(rng, 1))
    else:
        K.run_reduce(e, rng.normal(size=(1, 32, 9, 13)).astype(np.float32), K.make_w_last(rng, 1))


def _gconv_entry():
    import test_hip_generic_kernels as K
    K.check_conv(_L(), 8, 8, (1, 5, 7), 1)


TEMPORARIES = ("xsd_sw_test_gemm fp32", "xsd_sw_test_gemm bf16x6", "xsd_sw_test_gemm conv3", "xsd_swinir_test_nearest_conv",
               "xsd_hat_test_channel_mean", "xsd_hat_test_ca_combine", "xsd_swinir_test_pad with a mean", "xsd_swinir_test_pad without",
               "xsd_loss_test_scale", "xsd_test_conv3x3 fp32", "xsd_test_conv3x3 f16x3", "xsd_test_conv3x3_bwd fp32", "xsd_test_conv3x3_bwd f16x3",
               "xsd_test_conv3x3_ex bf16x6", "xsd_test_conv3x3_ex f16x3", "xsd_test_edge_expand", "xsd_test_edge_reduce", "xsd_restormer_test_pw",
               "xsd_restormer_test_attention", "xsd_restormer_test_attention_wide", "xsd_sw_test_gemm_view", "xsd_swinir_test_gemm_view",
               "xsd_probe_mfma_stream", "xsd_test_gconv")


@pytest.mark.parametrize("name", TEMPORARIES)
def test_entries_that_own_temporaries_free_what_they_allocate(name):
    """per call allocs == frees, and the count is the one read off the entry's code (DESIGN section 31 lists them)"""
    call, owns = _temporaries()[name]
    with window():
        call()
        torch.cuda.synchronize()
        s = stats()
        call()
        torch.cuda.synchronize()
        t = stats()
        assert t["allocs"] - s["allocs"] == t["frees"] - s["frees"] and live(t) == live(s)
        assert t["allocs"] - s["allocs"] == owns if owns is not None else t["allocs"] > s["allocs"]


# ---- c. the fsim plan cache -------------------------------------------------------------------------------------------------
def _plan_cost(h, w):
    """(blocks, bytes) of one plan (csrc/fsim.hip get_plan): the h x h DFT matrix of double2, the w x w one unless h == w (shared),
    NF filters of h x w doubles"""
    return (2 if h == w else 3), 16 * h * h + (0 if h == w else 16 * w * w) + 8 * FSIM_NF * h * w


def test_fsim_plan_cache_holds_exactly_the_most_recent_sizes():
    from xmm_superres_denoise.engine.engine import FsimEngine
    sizes = [(24, 24), (16, 16), (16, 20), (20, 16), (20, 24), (24, 20)]      # the largest first: the workspace is allocated once
    with window() as s0:
        e = FsimEngine()
        assert live() == live(s0)                                # create allocates nothing on the device
        first, lru, ws = {}, [], None
        for hw in sizes + sizes:
            r = e.eval(rand((1,) + hw), rand((1,) + hw, 1))
            torch.cuda.synchronize()
            if hw in lru:
                lru.remove(hw)
            lru.append(hw)
            del lru[:-FSIM_PLANS]
            blocks, nbytes = (sum(v) for v in zip(*(_plan_cost(*s) for s in lru)))
            now = stats()
            if ws is None:
                ws = now["live_bytes"] - s0["live_bytes"] - nbytes
                assert ws > 0
            assert now["live_blocks"] - s0["live_blocks"] == blocks + 1, (hw, lru)
            assert now["live_bytes"] - s0["live_bytes"] == nbytes + ws, (hw, lru)
            if hw in first:
                assert torch.equal(r, first[hw]), hw             # an evicted size, rebuilt: its first result bit for bit
            else:
                first[hw] = r.clone()
        # two alternating sizes allocate nothing after their first visit
        a, b = sizes[1], sizes[2]
        for hw in (a, b):
            e.eval(rand((1,) + hw), rand((1,) + hw, 1))
        torch.cuda.synchronize()
        s = stats()
        for hw in (a, b, a, b):
            assert torch.equal(e.eval(rand((1,) + hw), rand((1,) + hw, 1)), first[hw])
        torch.cuda.synchronize()
        assert moved(stats()) == moved(s)
        drop(e)
        assert live() == live(s0)


# ---- d. simulated refusals, swept -------------------------------------------------------------------------------------------
def _refused_call(call):
    """arm is set by the caller; the call must answer XSD_ERR_NOMEM with a message, and exactly one allocation was refused"""
    from xmm_superres_denoise.engine import XsdError
    r0 = stats()["refused"]
    with pytest.raises(XsdError) as ei:
        call()
    _L().xsd_test_mem_refuse(0)
    assert code_of(ei) == ERR_NOMEM, str(ei.value)
    assert _L().xsd_last_error()
    assert stats()["refused"] == r0 + 1


def sweep_growth(fam, prior, shape, run=None, expect=None):
    """Refuse, one at a time, each of the N allocations the call at `shape` makes on a handle that holds `prior` (None: a fresh handle).
    After each refusal: the held shape still gives its first result, the refused call repeated gives a fresh handle's result, both bit
    for bit, and destroy returns to the baseline.  Returns N."""
    run = run or fam.run
    L = _L()
    with window() as s0:
        ref = fam.fresh()
        want = run(ref, shape).clone()
        drop(ref)
        want_prior = None
        if prior:
            ref = fam.fresh()
            want_prior = run(ref, prior).clone()
            drop(ref)
        e = fam.fresh()
        if prior:
            run(e, prior)
        torch.cuda.synchronize()
        L.xsd_test_mem_refuse(0)
        run(e, shape)
        torch.cuda.synchronize()
        N = int(L.xsd_test_mem_refuse(0))
        drop(e)
        assert live() == live(s0)
        assert N >= 1 and (expect is None or N == expect), N
        for n in range(1, N + 1):
            e = fam.fresh()
            if prior:
                assert torch.equal(run(e, prior), want_prior)
            torch.cuda.synchronize()
            L.xsd_test_mem_refuse(n)
            _refused_call(lambda: run(e, shape))
            if prior:
                assert torch.equal(run(e, prior), want_prior), n
            assert torch.equal(run(e, shape), want), n
            drop(e)
            assert live() == live(s0), n
    return N


def _cfg_of(module, monkeypatch):
    """the C configuration struct a module's _make_engine would hand to its create, captured without creating"""
    from xmm_superres_denoise.engine import engine as E
    got = {}
    with monkeypatch.context() as mp:
        mp.setattr(E._ForwardEngine, "_create", lambda self, cfg, *a: got.setdefault("cfg", cfg))
        e = module._make_engine()
        e.h = None
    return got["cfg"]


def _creates(monkeypatch):
    from xmm_superres_denoise.engine import _lib
    from xmm_superres_denoise.models import HAT, Restormer, SwinFIR, SwinIR
    L = _L()

    def rrdb(kind, cin, cout, nf, nup):
        return _lib.XsdConfig(kind={"dn": 0, "sr": 1}[kind], in_channels=cin, out_channels=cout, num_filters=nf, num_res_blocks=1, num_upsample=nup,
                              memory_efficient=0, reserved=0)
    loss_cfg = _lib.XsdLossConfig(1.0, 0.0, 0.5, 0.5, 0.0, 0.0, 2.5, 0.01, 0.05, 13)
    two = lambda fn: (lambda cfg, h: fn(h))       # noqa: E731  (creates without a configuration)
    # name -> (create, destroy, configuration, device allocations of the create: read off the create functions)
    return {
        "xsd_create plane": (L.xsd_create, L.xsd_destroy, rrdb("dn", 1, 1, 32, 0), 13),
        "xsd_create plane sr": (L.xsd_create, L.xsd_destroy, rrdb("sr", 1, 1, 32, 1), 13),
        "xsd_create padded": (L.xsd_create, L.xsd_destroy, rrdb("dn", 1, 1, 48, 0), 16),
        "xsd_create generic": (L.xsd_create, L.xsd_destroy, rrdb("dn", 9, 9, 8, 0), 5),          # no conv is 16 wide both ways: no block-packed copy
        "xsd_create generic wide": (L.xsd_create, L.xsd_destroy, rrdb("dn", 9, 9, 16, 0), 6),
        "xsd_loss_create": (L.xsd_loss_create, L.xsd_loss_destroy, loss_cfg, 0),
        "xsd_ext_metrics_create": (two(L.xsd_ext_metrics_create), L.xsd_ext_metrics_destroy, None, 0),
        "xsd_fsim_create": (two(L.xsd_fsim_create), L.xsd_fsim_destroy, None, 0),
        "xsd_restormer_create": (L.xsd_restormer_create, L.xsd_restormer_destroy, _cfg_of(Restormer(**gr.full_cfg(**RESTORMER)), monkeypatch), 1),
        "xsd_swinfir_create": (L.xsd_swinfir_create, L.xsd_swinfir_destroy, _cfg_of(SwinFIR(**gs.full_cfg(**SWINFIR)), monkeypatch), 2),
        "xsd_hat_create": (L.xsd_hat_create, L.xsd_hat_destroy, _cfg_of(HAT(**gh.full_cfg(**HAT_A)), monkeypatch), 2),
        "xsd_swinir_create": (L.xsd_swinir_create, L.xsd_swinir_destroy, _cfg_of(SwinIR(**gi.full_cfg(**SWINIR_DN)), monkeypatch), 2),
    }


CREATES = ("xsd_create plane", "xsd_create plane sr", "xsd_create padded", "xsd_create generic", "xsd_create generic wide", "xsd_loss_create",
           "xsd_ext_metrics_create", "xsd_fsim_create", "xsd_restormer_create", "xsd_swinfir_create", "xsd_hat_create", "xsd_swinir_create")


@pytest.mark.parametrize("name", CREATES)
def test_every_refused_allocation_of_a_create_answers_nomem_and_leaks_nothing(name, monkeypatch):
    create, destroy, cfg, expect = _creates(monkeypatch)[name]
    L = _L()

    def make():
        h = ctypes.c_void_p(SENTINEL)
        rc = create(ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(h))
        return rc, h
    with window() as s0:
        L.xsd_test_mem_refuse(0)
        rc, h = make()
        N = int(L.xsd_test_mem_refuse(0))
        assert rc == OK and h.value not in (None, SENTINEL), L.xsd_last_error()
        assert stats()["live_blocks"] - s0["live_blocks"] == N
        destroy(h)
        assert live() == live(s0)
        assert N == expect
        for n in range(1, N + 1):
            r0 = stats()["refused"]
            L.xsd_test_mem_refuse(n)
            rc, h = make()
            L.xsd_test_mem_refuse(0)
            assert rc == ERR_NOMEM, (n, rc, L.xsd_last_error())
            assert L.xsd_last_error()
            assert h.value == SENTINEL, n                     # the handle pointer is untouched
            assert stats()["refused"] == r0 + 1
            assert live() == live(s0), n


# (family, held shape or None = fresh handle, shape of the refused call, which run, allocations of that call read off the code)
GROWTHS = {
    "xsd_forward first call fp32": ("rrdb nf32 fp32", None, "small", "run", 1),
    "xsd_forward ws growth f16x3": ("rrdb nf32 f16x3", "small", "large", "run", 1),
    "xsd_forward ws growth padded": ("rrdb nf48 padded f16x3", "small", "large", "run", 1),
    "xsd_forward ws growth generic": ("rrdb generic width", "small", "large", "run", 1),
    "training plan growth f16x3": ("rrdb nf32 f16x3", "small", "large", "train", 1),
    "training plan growth generic": ("rrdb generic width", "small", "large", "train", 1),
    "loss workspace first": ("loss", None, "small", "run", 1),
    "loss workspace growth": ("loss", "small", "large", "run", 1),
    "ext metrics workspace first": ("ext metrics", None, "small", "run", 1),
    "ext metrics workspace growth": ("ext metrics", "small", "large", "run", 1),
    "fsim first: two plan uploads and reserve": ("fsim", None, "small", "run", 3),
    "fsim growth: three plan uploads and reserve": ("fsim", "small", "large", "run", 4),
    "restormer first": ("restormer", None, "small", "run", 1),
    "restormer growth": ("restormer", "small", "large", "run", 1),
    "swinfir first: workspace and twiddles": ("swinfir fp32", None, "small", "run", 2),
    "swinfir bf16x6 first: wt3, workspace, twiddles": ("swinfir bf16x6", None, "small", "run", 3),
    "swinfir growth: workspace and twiddles": ("swinfir fp32", "small", "large", "run", 2),
    "swinfir smaller shape: twiddles alone": ("swinfir fp32", "large", "small", "run", 1),
    "hat bf16x6 first: wt3 and workspace": ("hat bf16x6", None, "small", "run", 2),
    "hat growth": ("hat fp32", "small", "large", "run", 1),
    "swinir bf16x6 first: wt3 and workspace": ("swinir bf16x6", None, "small", "run", 2),
    "swinir growth": ("swinir fp32", "small", "large", "run", 1),
}


@pytest.mark.parametrize("name", list(GROWTHS))
def test_every_refused_allocation_of_a_growth_path_leaves_the_handle_usable(name):
    fam_name, prior, shape, which, expect = GROWTHS[name]
    fam = FAMS[fam_name]()
    sweep_growth(fam, getattr(fam, prior) if prior else None, getattr(fam, shape), run=getattr(fam, which), expect=expect)


def test_fsim_eviction_whose_rebuild_is_refused_keeps_the_other_plans():
    """XSD_FSIM_PLANS sizes are cached; a fifth evicts the least recently used one BEFORE its own plan is uploaded.  With each of
    those uploads refused in turn: the three younger sizes still give their first results without an allocation, the evicted and the
    refused size are rebuilt to their first results, destroy returns to the baseline."""
    from xmm_superres_denoise.engine.engine import FsimEngine
    sizes = [(24, 24), (16, 16), (16, 20), (20, 16), (20, 24)]
    ev = lambda e, hw: e.eval(rand((1,) + hw), rand((1,) + hw, 1))      # noqa: E731
    with window() as s0:
        for n in (1, 2, 3):
            e = FsimEngine()
            first = {hw: ev(e, hw).clone() for hw in sizes[:4]}
            ref = FsimEngine()
            first[sizes[4]] = ev(ref, sizes[4]).clone()
            drop(ref)
            torch.cuda.synchronize()
            _L().xsd_test_mem_refuse(n)
            _refused_call(lambda: ev(e, sizes[4]))
            s = stats()
            for hw in sizes[1:4]:
                assert torch.equal(ev(e, hw), first[hw]), (n, hw)
            torch.cuda.synchronize()
            assert moved(stats()) == moved(s), n                   # still cached: nothing was rebuilt
            for hw in (sizes[0], sizes[4]):
                assert torch.equal(ev(e, hw), first[hw]), (n, hw)
            drop(e)
            assert live() == live(s0), n


def test_max_abs_slot_array_growth_refused_in_the_hooks_library():
    """the slot-array growth of ensure_plan needs XSD_TEST_AMAX_CAP (hooks library): swept in a child process, as
    test_hip_network.py::test_max_abs_slot_array_grows_without_changing_results runs it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = os.path.join(root, "xmm-superres-denoise_amd", "lib", "libxsd_hip_hooks.so")
    assert os.path.exists(hooks), "build the hooks variant: make -C xmm-superres-denoise_amd/csrc hooks (__graft_entry__.build() does)"
    env = dict(os.environ, XSD_LIB=hooks, XSD_TEST_AMAX_CAP="128")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "lifetime_amax_worker.py"), root], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "slot array sweep OK: N = 2" in out, out[-3000:]


# ---- e. the Python side -----------------------------------------------------------------------------------------------------
def _train_step(m, opt, x, t):
    y = m(x)
    loss = F.l1_loss(y, t)
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=False)


def _py_cases():
    from xmm_superres_denoise.models import (HAT, GeneratorRRDB_DN, Restormer, SwinFIR, SwinIR, TrainableSwinFIR, TrainableSwinIR)

    def trainer(make, shape, out_scale=1):
        def build():
            torch.manual_seed(21)
            m = make().cuda().train()
            opt = torch.optim.Adam(m.parameters(), lr=1e-4)
            x = rand(shape)
            t = rand((shape[0], shape[1], shape[2] * out_scale, shape[3] * out_scale), 1)
            return m, (lambda: _train_step(m, opt, x, t)), x
        return build

    def evaluator(make, shape):
        def build():
            torch.manual_seed(21)
            m = make().cuda().eval()
            x = rand(shape)

            def step():
                with torch.no_grad():
                    m(x)
            return m, step, x
        return build
    return {
        "GeneratorRRDB fp32": trainer(lambda: GeneratorRRDB_DN(1, 1, 8, 1).set_math("fp32"), (2, 1, 16, 16)),
        "GeneratorRRDB bf16x6": trainer(lambda: GeneratorRRDB_DN(1, 1, 8, 1).set_math("bf16x6"), (2, 1, 16, 16)),
        "GeneratorRRDB f16x3": trainer(lambda: GeneratorRRDB_DN(1, 1, 8, 1).set_math("f16x3"), (2, 1, 16, 16)),
        "GeneratorRRDB memory_efficient": trainer(lambda: GeneratorRRDB_DN(1, 1, 8, 1, memory_efficient=True).set_math("f16x3"), (2, 1, 16, 16)),
        "Restormer": evaluator(lambda: Restormer(**gr.full_cfg(**RESTORMER)), (1, 1, 8, 8)),
        "SwinFIR": evaluator(lambda: SwinFIR(**gs.full_cfg(**SWINFIR)), (1, 1, 8, 12)),
        "HAT": evaluator(lambda: HAT(**gh.full_cfg(**HAT_A)), (1, 1, 16, 16)),
        "SwinIR": evaluator(lambda: SwinIR(**gi.full_cfg(**SWINIR_DN)), (1, 1, 8, 12)),
        "TrainableSwinIR": trainer(lambda: TrainableSwinIR(SwinIR(**gi.full_cfg(**SWINIR_DN)).cuda()), (2, 1, 18, 21)),
        "TrainableSwinFIR": trainer(lambda: TrainableSwinFIR(SwinFIR(**gs.full_cfg(**SWINFIR_1CONV)).cuda()), (2, 1, 8, 12), 2),
    }


PY_CASES = ("GeneratorRRDB fp32", "GeneratorRRDB bf16x6", "GeneratorRRDB f16x3", "GeneratorRRDB memory_efficient", "Restormer", "SwinFIR", "HAT",
            "SwinIR", "TrainableSwinIR", "TrainableSwinFIR")
ENGINE_BACKED = PY_CASES[:8]


def _warm(build):
    """one build and step outside the measured window: the cached inputs and whatever torch creates lazily at a first use exist"""
    m, step, x = build()
    step()
    torch.cuda.synchronize()
    del m, step, x
    gc.collect()


@pytest.mark.parametrize("name", PY_CASES)
def test_a_dropped_module_leaves_both_allocators_at_the_baseline_and_steps_are_steady(name):
    """built, stepped five times, dropped: the ledger and torch.cuda.memory_allocated() are back where they were; steps 3, 4 and 5 end
    at the same memory_allocated() and move no ledger counter"""
    build = _py_cases()[name]
    _warm(build)
    with window() as s0:
        mem0 = torch.cuda.memory_allocated()
        m, step, x = build()
        step()
        step()
        torch.cuda.synchronize()
        s, mem = stats(), torch.cuda.memory_allocated()
        if name in ENGINE_BACKED:
            assert s["live_blocks"] > s0["live_blocks"]
        for _ in range(3):
            step()
            torch.cuda.synchronize()
            assert moved(stats()) == moved(s) and torch.cuda.memory_allocated() == mem
        del m, step, x
        gc.collect()
        torch.cuda.synchronize()
        assert live() == live(s0)
        assert torch.cuda.memory_allocated() == mem0


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("name", PY_CASES)
def test_a_copy_of_a_used_module_owns_its_allocations(name, how):
    """the copy creates its own handle at its first forward; dropping it returns exactly its share to the ledger and to torch's
    allocator, the original keeps what it held.  The trainable Swin nets hold no handle: their copies move no ledger counter."""
    build = _py_cases()[name]
    _warm(build)
    with window() as s0:
        mem0 = torch.cuda.memory_allocated()
        m, step, x = build()
        step()
        with torch.no_grad():
            ym = m(x)
        torch.cuda.synchronize()
        own, mem_own = stats(), torch.cuda.memory_allocated()
        backed = name in ENGINE_BACKED
        assert (own["live_blocks"] > s0["live_blocks"]) == backed
        c = copy.deepcopy(m) if how == "deepcopy" else pickle.loads(pickle.dumps(m))
        assert live() == live(own) and torch.cuda.memory_allocated() > mem_own      # its own parameters; its handle at its first forward
        with torch.no_grad():
            yc = c(x)
        torch.cuda.synchronize()
        assert torch.equal(yc, ym)
        both = stats()
        if backed:
            assert both["live_blocks"] - own["live_blocks"] == own["live_blocks"] - s0["live_blocks"]      # the same handle again,
            assert 0 < both["live_bytes"] - own["live_bytes"] <= own["live_bytes"] - s0["live_bytes"]      # its workspace planned for x alone
        else:
            assert moved(both) == moved(own)
        del c, yc
        gc.collect()
        torch.cuda.synchronize()
        assert live() == live(own) and torch.cuda.memory_allocated() == mem_own
        del m, step, ym, x
        gc.collect()
        torch.cuda.synchronize()
        assert live() == live(s0) and torch.cuda.memory_allocated() == mem0


@pytest.mark.parametrize("name", ENGINE_BACKED)
def test_load_state_dict_and_repack_allocate_nothing(name):
    build = _py_cases()[name]
    with window():
        m, step, x = build()
        step()
        step()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        torch.cuda.synchronize()
        s = stats()
        m.load_state_dict(sd)
        step()
        torch.cuda.synchronize()
        assert moved(stats()) == moved(s)
        del m, step, x
        gc.collect()


@pytest.mark.parametrize("which", ["loss", "ext metrics", "fsim"])
def test_a_dropped_loss_or_metric_engine_returns_everything(which):
    """three evaluations, then dropped: the ledger and torch.cuda.memory_allocated() are back at the baseline; the second and third
    evaluation end at the same memory_allocated().  A deep copy and an unpickled loss own their handles and return them."""
    fam = FAMS[which]()
    e = fam.fresh()
    fam.run(e, fam.small)       # outside the window: the cached inputs exist
    torch.cuda.synchronize()
    del e
    with window() as s0:
        mem0 = torch.cuda.memory_allocated()
        e = fam.fresh()
        mems = []
        for _ in range(3):
            fam.run(e, fam.small)
            torch.cuda.synchronize()
            mems.append(torch.cuda.memory_allocated())
        assert mems[1] == mems[2] == mem0       # the results are dropped; the workspace is the library's, not torch's
        own = stats()
        assert own["live_blocks"] > s0["live_blocks"]
        if which == "loss":
            for clone in (copy.deepcopy, lambda o: pickle.loads(pickle.dumps(o))):
                c = clone(e)
                assert live() == live(own)      # a workspace comes with the first evaluation
                assert torch.equal(fam.run(c, fam.small), fam.run(e, fam.small))
                torch.cuda.synchronize()
                both = stats()
                assert both["live_blocks"] - own["live_blocks"] == own["live_blocks"] - s0["live_blocks"]
                assert both["live_bytes"] - own["live_bytes"] == own["live_bytes"] - s0["live_bytes"]
                del c
                gc.collect()
                torch.cuda.synchronize()
                assert live() == live(own) and torch.cuda.memory_allocated() == mem0
        del e
        gc.collect()
        torch.cuda.synchronize()
        assert live() == live(s0) and torch.cuda.memory_allocated() == mem0


def test_a_refused_stamp_buffer_answers_nomem_and_the_handle_stays_usable():
    """xsd_debug_stamps(e, 1) is the one allocation outside the creates and growth paths: refused, it answers XSD_ERR_NOMEM like them,
    the engine computes what it computed before, stamps can be enabled afterwards, and destroy returns everything"""
    fam = FAMS["rrdb nf32 f16x3"]()
    L = _L()
    with window() as s0:
        e = fam.fresh()
        want = fam.run(e, fam.small).clone()
        torch.cuda.synchronize()
        held, r0 = stats(), stats()["refused"]
        L.xsd_test_mem_refuse(1)
        rc = L.xsd_debug_stamps(e.h, 1, None)
        assert L.xsd_test_mem_refuse(0) == 1                     # the one allocation of that call
        assert rc == ERR_NOMEM and L.xsd_last_error() and stats()["refused"] == r0 + 1
        assert live() == live(held)
        assert torch.equal(fam.run(e, fam.small), want)
        _assert_ok(L.xsd_debug_stamps(e.h, 1, None))
        assert stats()["live_blocks"] == held["live_blocks"] + 1
        assert torch.equal(fam.run(e, fam.small), want)
        drop(e)
        assert live() == live(s0)
