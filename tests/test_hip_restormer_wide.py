"""The Restormer engine's wide channel attention (csrc/restormer.hip: rst_wgram_kernel, rst_wsoftmax_kernel, rst_wfold_kernel; 65 to 128
channels per head) through its test hook (include/xsd.h: xsd_restormer_test_attention_wide) against a plain float64 reference, bit for
bit against the narrow kernels on widths both take, for a fixed order and batch locality, and its refusals; then whole networks that
run it: the reference's goldens of the published dim 48 and of dim 64 (the 128-channel cap), a shallow dim 48 at 64 x 64 against the
float64 restatement, a shape change on one module, and the checkpoint -> load_model(dim=48) -> infer_file path.  The yardstick is the
same reference in fp32 (on the same device, or the reference's own fp32 output), the bar the project's 2x.  Every hook output goes into
a NaN-filled buffer with sentinel words behind it."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import gen_restormer_wide as gw
import restormer_torch as rt

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = 12345.0


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    y, y32, y64 = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (y, y32, y64))
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


def _guarded(shape, guard=300):
    """a NaN-filled contiguous tensor of `shape` with `guard` sentinel elements behind it in the same allocation"""
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), SENTINEL, device="cuda")
    buf[:n] = float("nan")
    return buf[:n].view(shape), buf[n:]


def _untouched(guard):
    return bool(torch.all(guard == SENTINEL))


def _d(t):
    return None if t is None else t.double()


def _attn_inputs(B, C, heads, HW):
    g = torch.Generator().manual_seed(10000 * C + 100 * heads + HW)
    qkv = torch.randn(B, 3 * C, HW, generator=g).cuda()
    temp = torch.rand(heads, generator=g) * 1.5 + 0.5
    if heads > 1:
        temp[-1] = -temp[-1]
    wpo = ((torch.rand(C, C, generator=g) * 2 - 1) / C ** 0.5).cuda()
    bpo = ((torch.rand(C, generator=g) * 2 - 1)).cuda() if heads > 1 else None
    x = torch.randn(B, C, HW, generator=g).cuda()
    return qkv, temp.cuda(), wpo, bpo, x


def _attn_reference(qkv, temp, wpo, bpo, x, heads):
    B, C, HW = x.shape
    o = rt.channel_attention(qkv.view(B, 3 * C, HW, 1), temp.view(heads, 1, 1), heads).view(B, C, HW)
    y = torch.matmul(wpo, o)
    return x + (y if bpo is None else y + bpo[:, None])


def _run(fn, qkv, temp, wpo, bpo, x, heads, what, finite=True):
    xs, guard = _guarded(tuple(x.shape))
    xs.copy_(x)
    fn(qkv, temp, wpo, bpo, xs, heads)
    assert _untouched(guard), what
    if finite:
        assert torch.isfinite(xs).all(), what
    return xs


WIDE_CASES = [
    (2, 65, 1, 70),          # the first width past the old limit: a 2 x 2 tile grid with one row in the second tiles
    (1, 96, 1, 1500),        # the published width, a second pixel range of 476 pixels
    (1, 128, 1, 1025),       # the cap, a last range of one pixel
    (2, 192, 2, 64),         # 96 channels per head with a head offset
    (1, 130, 2, 3),          # fewer pixels than one 64-pixel round
    (1, 128, 1, 1),          # F.normalize of one-element rows
]


@pytest.mark.parametrize("B,C,heads,HW", WIDE_CASES)
def test_wide_channel_attention_against_float64(B, C, heads, HW):
    from xmm_superres_denoise.engine import restormer_channel_attention_wide as wide
    qkv, temp, wpo, bpo, x = _attn_inputs(B, C, heads, HW)
    if HW == 1025:
        qkv[0, 70] = 0           # a q channel (of the second tile row) that is zero over the whole image: its norm is clamped at 1e-12
    what = f"wide channel attention {B} x {C} ({heads} heads) x {HW}"
    y = _run(wide, qkv, temp, wpo, bpo, x, heads, what)
    y64 = _attn_reference(qkv.double(), temp.double(), wpo.double(), _d(bpo), x.double(), heads)
    y32 = _attn_reference(qkv, temp, wpo, bpo, x, heads)
    _assert_within_2x_of_fp32(y, y32, y64, what)
    assert torch.equal(_run(wide, qkv, temp, wpo, bpo, x, heads, what), y)                       # two runs: bit for bit
    for i in range(B if B > 1 else 0):
        one = _run(wide, qkv[i:i + 1].contiguous(), temp, wpo, bpo, x[i:i + 1].contiguous(), heads, what)
        assert torch.equal(one[0], y[i]), i                                                      # each image = its own B = 1 run


@pytest.mark.parametrize("B,C,heads,HW", [(2, 64, 1, 1500), (1, 40, 8, 3000), (1, 6, 6, 70)])
def test_wide_kernels_equal_the_narrow_kernels_bit_for_bit(B, C, heads, HW):
    """the same operations in the same order, entry by entry: on a width both paths take the outputs are equal, not close"""
    from xmm_superres_denoise.engine import restormer_channel_attention as narrow, restormer_channel_attention_wide as wide
    qkv, temp, wpo, bpo, x = _attn_inputs(B, C, heads, HW)
    what = f"wide against narrow {B} x {C} ({heads} heads) x {HW}"
    yw = _run(wide, qkv, temp, wpo, bpo, x, heads, what)
    yn = _run(narrow, qkv, temp, wpo, bpo, x, heads, what)
    assert torch.equal(yw, yn), (what, float((yw - yn).abs().max()))
    assert not torch.equal(yw, x)


def test_wide_channel_attention_keeps_a_nan_in_its_image():
    from xmm_superres_denoise.engine import restormer_channel_attention_wide as wide
    B, C, heads, HW = 2, 96, 1, 1500
    qkv, temp, wpo, bpo, x = _attn_inputs(B, C, heads, HW)
    clean = _run(wide, qkv, temp, wpo, bpo, x, heads, "clean")
    qn = qkv.clone()
    qn[1, C + 70, 1234] = float("nan")       # a k channel of image 1, in its second pixel range
    dirty = _run(wide, qn, temp, wpo, bpo, x, heads, "dirty", finite=False)
    assert not torch.isfinite(dirty[1]).all()
    assert torch.equal(dirty[0], clean[0])


def _z(*shape):
    return torch.zeros(*shape, device="cuda")


def test_wide_channel_attention_refusals():
    from xmm_superres_denoise.engine import XsdError, _lib, restormer_channel_attention_wide as wide
    x = torch.full((1, 129, 4), 7.0, device="cuda")
    with pytest.raises(XsdError, match="Restormer wide attention test: 129 channels per head; the wide kernels take at most 128"):
        wide(_z(1, 387, 4), _z(1), _z(129, 129), None, x, 1)
    assert torch.all(x == 7.0)                                       # refused before any launch
    with pytest.raises(XsdError, match="3 heads do not divide 10 channels"):
        wide(_z(1, 30, 4), _z(3), _z(10, 10), None, _z(1, 10, 4), 3)
    with pytest.raises(XsdError, match=r"Restormer wide attention test: 65536 images are outside \[1, 65535\]"):
        wide(_z(65536, 3, 1), _z(1), _z(1, 1), None, _z(65536, 1, 1), 1)
    L, t = _lib.load(), _z(64)
    p = t.data_ptr()
    assert L.xsd_restormer_test_attention_wide(p, p, p, None, p, 1, 8320, 65, 4, None) != 0
    assert b"8320 channels are outside [1, 8192]" in L.xsd_last_error()
    assert L.xsd_restormer_test_attention_wide(p, p, p, None, p, 1, 4, 1, 0, None) != 0
    assert b"0 pixels are outside [1, 2^28]" in L.xsd_last_error()
    assert L.xsd_restormer_test_attention_wide(p, p, p, None, p, 1, 4, 0, 4, None) != 0
    assert b"0 heads do not divide 4 channels" in L.xsd_last_error()
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.xsd_restormer_test_attention_wide(a[0], a[1], a[2], None, a[3], 1, 4, 2, 4, None) != 0
        assert b"null argument" in L.xsd_last_error()
    assert torch.all(t == 0)


# ---------------------------------------------------------------------------------------------------------------
# whole networks past 64 channels per head
# ---------------------------------------------------------------------------------------------------------------
def _module(cfg, state):
    from xmm_superres_denoise.models import Restormer
    m = Restormer(**gw.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return m.cuda()


@pytest.mark.parametrize("case", list(gw.CASES))
def test_parity_with_the_wide_reference_goldens(case):
    z = np.load(os.path.join(G, f"restormer_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    m = _module(cfg, gw.make_state(cfg, int(z["seed"])))
    with torch.no_grad():
        y = m(torch.from_numpy(z["x"]).cuda()).cpu().numpy()
    assert y.shape == z["y64"].shape
    _assert_within_2x_of_fp32(y, z["y32"], z["y64"], case)


SHALLOW48 = dict(inp_channels=3, out_channels=3, dim=48, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1)


@pytest.fixture(scope="module")
def shallow48():
    state = gw.make_state(SHALLOW48, 71)
    return _module(SHALLOW48, state), state


def test_shallow_dim48_against_float64_restatement_and_batch_isolation(shallow48):
    m, state = shallow48
    x = torch.from_numpy(gw.make_input((2, 3, 64, 64), 72)).cuda()
    full = gw.full_cfg(**SHALLOW48)
    with torch.no_grad():
        y = m(x)
        y64 = rt.restormer_forward({k: torch.from_numpy(v).cuda().double() for k, v in state.items()}, x.double(), **full)
        y32 = rt.restormer_forward({k: torch.from_numpy(v).cuda() for k, v in state.items()}, x, **full)
        singles = [m(x[i:i + 1].contiguous()) for i in range(2)]
        y2 = m(x)
    assert y.shape == y64.shape == (2, 3, 64, 64)
    _assert_within_2x_of_fp32(y, y32, y64, "Restormer dim 48, depths 1, 2 x 3 x 64 x 64")
    assert torch.equal(y, y2)
    for i in range(2):
        assert torch.equal(y[i:i + 1], singles[i]), i


def test_shape_change_on_one_module_gives_the_first_result_again(shallow48):
    m, _ = shallow48
    xa = torch.from_numpy(gw.make_input((1, 3, 16, 24), 73)).cuda()
    xb = torch.from_numpy(gw.make_input((2, 3, 64, 64), 74)).cuda()
    with torch.no_grad():
        ya = m(xa).clone()
        yb = m(xb).clone()               # a larger workspace: re-planned
        ya2 = m(xa)
    assert torch.isfinite(ya).all() and torch.isfinite(yb).all()
    assert torch.equal(ya2, ya)


def test_load_model_dim48_and_infer_file_round_trip(tmp_path):
    from xmm_superres_denoise.infer import infer_file, load_model, read_fits, write_fits
    from xmm_superres_denoise.models import Model
    cfg = dict(inp_channels=1, out_channels=1, dim=48)          # what model_cfg("restormer", dim=48) builds: 96 channels on one head
    state = gw.make_state(cfg, 75)
    ck = os.path.join(tmp_path, "restormer48.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, ck)
    with pytest.raises(RuntimeError, match="size mismatch"):
        load_model(ck, "restormer", lr_res=64)                  # without dim= the factory builds dim 24: the shapes do not fit
    model = load_model(ck, "restormer", lr_res=64, dim=48)
    assert isinstance(model, Model) and model.model.dim == 48
    for k, v in model.model.state_dict().items():
        assert torch.equal(v.cpu(), torch.from_numpy(state[k])), k
    counts = np.random.default_rng(5).poisson(0.3, size=(59, 61)).astype(np.float32)
    src = os.path.join(tmp_path, "P0001_detxy.fits")
    write_fits(src, counts, OrderedDict(CRPIX1=30.5, CRPIX2=29.5, EXPOSURE=10000.0))
    pred, out_path = infer_file(src, model, None, os.path.join(tmp_path, "out"), lr_res=64)
    back, _ = read_fits(out_path)
    assert pred.shape == (64, 64) and np.isfinite(pred).all() and out_path.endswith("_dn_predict.fits.gz")
    assert np.array_equal(back.astype(np.float32), pred.astype(np.float32))
