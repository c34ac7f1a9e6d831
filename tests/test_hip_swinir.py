"""SwinIR forward on the MI355X engine (csrc/swinir.hip) through the drop-in module, against the reference's goldens and the float64
restatement (tests/golden/swinir_torch.py): parity of all four heads in both math modes, the reflect pad and the nearest-2x conv on their
own, batch isolation, determinism and NaN containment, workspace re-planning, the checkpoint / infer.py path, parameter re-packing,
copies, and the refusals."""
import copy
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_swinir as gi
import swinir_torch as si

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -12345.0


def _module(cfg, state, device="cuda"):
    from xmm_superres_denoise.models import SwinIR
    m = SwinIR(**gi.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return m.to(device)


def _sd(state, device, dtype):
    return {k: torch.from_numpy(v).to(device, dtype if v.dtype == np.float32 else None) for k, v in state.items()}


def _errs(y, ref):
    e = np.abs(np.asarray(y, np.float64) - ref)
    return float(np.sqrt((e ** 2).mean())), float(e.max() / np.abs(ref).max())


def _assert_within_2x_of_fp32(y, y32, y64, what):
    rms, mx = _errs(y, y64)
    rms32, mx32 = _errs(y32, y64)
    print(f"{what}: engine rms {rms:.3e} max-rel {mx:.3e} | fp32 reference rms {rms32:.3e} max-rel {mx32:.3e}")
    assert rms <= 2 * rms32 and mx <= 2 * mx32, (what, rms, rms32, mx, mx32)


def _golden(case):
    z = np.load(os.path.join(G, f"swinir_{case}.npz"))
    cfg = json.loads(str(z["cfg"]))
    return z, cfg, gi.make_state(cfg, int(z["seed"]))


@pytest.mark.parametrize("case", list(gi.CASES))
def test_parity_with_reference_goldens_in_both_math_modes(case):
    z, cfg, state = _golden(case)
    m = _module(cfg, state)
    x = torch.from_numpy(z["x"]).cuda()
    with torch.no_grad():
        y = m(x)
        assert tuple(y.shape) == z["y64"].shape and y.is_contiguous()
        assert m._engine.out_size(*x.shape[2:]) == m.out_size(*x.shape[2:]) == tuple(y.shape[2:])
        _assert_within_2x_of_fp32(y.cpu().numpy(), z["y32"], z["y64"], f"{case} fp32")
        y6 = m.set_math("bf16x6")(x)
        assert m._engine.get_math() == "bf16x6" and tuple(y6.shape) == z["y64"].shape
        _assert_within_2x_of_fp32(y6.cpu().numpy(), z["y32"], z["y64"], f"{case} bf16x6")
        assert torch.equal(m.set_math("fp32")(x), y)          # back in fp32: bit for bit what it was before the module left fp32


@pytest.mark.parametrize("B,C,H,W,ws", [(2, 1, 13, 19, 8), (1, 3, 7, 10, 4), (1, 1, 8, 8, 4), (1, 1, 9, 15, 8), (1, 1, 403, 411, 8)])
def test_reflect_pad_alone_is_bitwise(B, C, H, W, ws):
    from xmm_superres_denoise.engine import swinir_pad
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * 1000 + W)).cuda()
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    mean, rng = (gi.RGB_MEAN, 255.0) if C == 3 else (None, 1.0 if H != 13 else 0.5)
    mt = torch.tensor(mean or [0.0] * C, device="cuda").view(1, C, 1, 1)
    ref = (F.pad(x, (0, pw, 0, ph), "reflect") - mt) * rng
    out = torch.full((B, C, H + ph, W + pw), SENTINEL, device="cuda")
    y = swinir_pad(x, ws, mean, rng, out=out)
    assert y.shape == ref.shape and torch.equal(y, ref)      # every element written, each bit for bit


@pytest.mark.parametrize("B,H,W,cin,N", [(1, 5, 7, 3, 5), (2, 8, 6, 16, 64), (1, 33, 17, 64, 64)])
def test_nearest_conv_alone_against_float64(B, H, W, cin, N):
    """lrelu(conv3x3(nearest2x(a))) against the same expression in float64; the bar is 2 x the error of the expression in torch fp32 on the
    device.  At K = 27 (the first shape) torch's fp32 result is all but correctly rounded (rms 3.41e-08, max-rel 4.64e-08), so the bar
    there is about one rounding: the engine's GEMM instance for SwinIR adds the bias to its double sum and rounds to fp32 once, and measures
    rms 5.88e-08, max-rel 9.02e-08 in fp32 and rms 3.89e-08, max-rel 8.41e-08 in bf16x6 against the bar of 6.82e-08 / 9.27e-08.  (With the
    two roundings of the SwinFIR / HAT instances -- sum, then + bias -- it measured 6.39e-08 / 1.115e-07 and missed the max-rel bar;
    torch's own CPU fp32 conv measures 6.86e-08 / 1.096e-07 on the same input.)"""
    from xmm_superres_denoise.engine import swinir_nearest_conv
    g = torch.Generator().manual_seed(1000 * H + cin)
    a = torch.randn(B, H, W, cin, generator=g).cuda()
    w = (torch.randn(N, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    an = a.permute(0, 3, 1, 2).contiguous()

    def expr(a_, w_, b_):
        y = F.leaky_relu(F.conv2d(F.interpolate(a_, scale_factor=2, mode="nearest"), w_, b_, padding=1), 0.2)
        return y.permute(0, 2, 3, 1).contiguous().cpu().numpy()

    ref64, ref32 = expr(an.double(), w.double(), b.double()), expr(an, w, b)
    n = B * 4 * H * W * N
    for math in ("fp32", "bf16x6"):
        buf = torch.full((n + 3 * N,), SENTINEL, device="cuda")
        y = swinir_nearest_conv(a, w, b, 0.2, math, out=buf[:n].view(B, 2 * H, 2 * W, N))
        assert torch.all(buf[n:] == SENTINEL) and not torch.any(y == SENTINEL), math
        _assert_within_2x_of_fp32(y.cpu().numpy(), ref32, ref64, f"nearest conv {B} x {H} x {W}, {cin} -> {N}, {math}")
    # each image of the batch equals its own B = 1 run
    for i in range(B):
        assert torch.equal(swinir_nearest_conv(a[i:i + 1].contiguous(), w, b, 0.2, "fp32")[0], swinir_nearest_conv(a, w, b, 0.2, "fp32")[i])


def test_mid_size_denoiser_against_the_float64_restatement():
    """embed 60, 2 x 2 blocks of 6 heads, window 8, 2 x 1 x 101 x 99 -> padded 104 x 104, no golden: the restatement in float64 on the
    device is the truth, the same restatement in fp32 (torch eager) the yardstick"""
    cfg = dict(img_size=64, patch_size=1, in_chans=1, embed_dim=60, depths=[2, 2], num_heads=[6, 6], window_size=8, upscale=1, upsampler="")
    state = gi.make_state(cfg, 2026)
    x = torch.from_numpy(gi.make_input((2, 1, 101, 99), 2027)).cuda()
    m = _module(cfg, state)
    with torch.no_grad():
        y = m(x).cpu().numpy()
        y64 = si.swinir_forward(_sd(state, "cuda", torch.float64), x.double(), **cfg).cpu().numpy()
        y32 = si.swinir_forward(_sd(state, "cuda", torch.float32), x, **cfg).cpu().numpy()
    assert y.shape == (2, 1, 101, 99)
    _assert_within_2x_of_fp32(y, y32, y64, "DN embed 60, 101 x 99")


@pytest.mark.parametrize("case", ["a_dn_reflect", "d_nearest_x2_rgb_pad"])
def test_batch_isolation_determinism_and_nan_containment(case):
    z, cfg, state = _golden(case)
    m = _module(cfg, state)
    _, C, H, W = z["x"].shape
    x = torch.from_numpy(gi.make_input((3, C, H, W), 77)).cuda()
    with torch.no_grad():
        y, y2 = m(x), m(x)
        singles = [m(x[i:i + 1].contiguous()) for i in range(3)]
        xn = x.clone()
        xn[1, 0, H - 2, 3] = float("nan")
        yn = m(xn)
        ref = si.swinir_forward(_sd(state, "cuda", torch.float64), xn[1:2].double(), **cfg)
    assert torch.equal(y, y2)                                      # two runs: bit for bit
    for i in range(3):
        assert torch.equal(y[i:i + 1], singles[i]), i              # each image = its own B = 1 run
    for i in (0, 2):
        assert torch.equal(yn[i], y[i]), i                         # the others do not see the NaN
    bad_ref, bad = ~torch.isfinite(ref[0]), ~torch.isfinite(yn[1])
    assert bad_ref.any() and bool((bad | ~bad_ref).all())          # every pixel the reference makes non-finite is non-finite here
    print(f"{case}: non-finite pixels: restatement {int(bad_ref.sum())}, engine {int(bad.sum())} of {bad.numel()}")


def test_workspace_growth_and_replan_are_bitwise_neutral():
    """a larger shape after a smaller one (a larger workspace and a new plan), then the smaller one again (a re-plan inside the workspace
    held), then a size that pads to the same padded size as the first: none leaves a trace in the outputs"""
    z, cfg, state = _golden("a_dn_reflect")
    m, fresh, fresh3 = _module(cfg, state), _module(cfg, state), _module(cfg, state)
    x1 = torch.from_numpy(gi.make_input((1, 1, 13, 19), 78)).cuda()
    x2 = torch.from_numpy(gi.make_input((2, 1, 30, 21), 79)).cuda()
    x3 = torch.from_numpy(gi.make_input((1, 1, 16, 24), 80)).cuda()      # the padded size of x1, without a pad
    with torch.no_grad():
        y1, y2, y1b, y3 = m(x1), m(x2), m(x1), m(x3)
        only2, only3 = fresh(x2), fresh3(x3)
    assert y1.shape == (1, 1, 13, 19) and y2.shape == (2, 1, 30, 21) and y3.shape == (1, 1, 16, 24)
    assert torch.equal(y1, y1b) and torch.equal(y2, only2) and torch.equal(y3, only3)


@pytest.mark.parametrize("head,upscale", [("", 1), ("pixelshuffle", 2)])
def test_load_swinir_from_a_lightning_checkpoint_and_infer_file(tmp_path, head, upscale):
    from xmm_superres_denoise.infer import infer_file, load_swinir, read_fits, write_fits
    cfg = dict(img_size=64, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=8, upscale=upscale, upsampler=head)
    state = gi.make_state(cfg, 31)
    ck = os.path.join(tmp_path, "swinir.ckpt")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in state.items()}}, ck)
    m = load_swinir(ck, math="bf16x6", **cfg)
    assert m.get_math() == "bf16x6" and next(m.parameters()).is_cuda
    bare = os.path.join(tmp_path, "bare.ckpt")
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, bare)
    m = load_swinir(bare, **cfg)
    assert m.get_math() == "fp32"
    for k, v in m.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), state[k]), k
    counts = np.random.default_rng(5).poisson(0.3, size=(403, 411)).astype(np.int32)
    src = os.path.join(tmp_path, "P0001_detxy.fits")
    hdr = OrderedDict(CRPIX1=200.5, CRPIX2=204.5, CDELT1=-0.001, CDELT2=0.001, PA_PNT=12.5, EXPOSURE=10000.0)
    blob = np.ascontiguousarray(counts, dtype=">i4")
    write_fits(src, counts.astype(np.float32), hdr)
    # the same file as 32-bit integers: rewrite the data unit and BITPIX in place
    raw = open(src, "rb").read()
    assert raw[80:160].startswith(b"BITPIX  =") and len(raw) % 2880 == 0
    card = ("BITPIX  = " + f"{32:>20d}").ljust(80).encode()
    head_len = len(raw) - (-(-blob.nbytes // 2880) * 2880)
    open(src, "wb").write(raw[:80] + card + raw[160:head_len] + blob.tobytes() + b"\0" * (-blob.nbytes % 2880))
    data, _ = read_fits(src)
    assert data.dtype.kind == "i" and np.array_equal(data, counts)
    pred, out_path = infer_file(src, m, None, os.path.join(tmp_path, "out"))
    back, h = read_fits(out_path)
    kind = "sr" if upscale > 1 else "dn"
    assert pred.shape == (416 * upscale, 416 * upscale) and np.isfinite(pred).all() and out_path.endswith(f"P0001_detxy_{kind}_predict.fits.gz")
    assert np.array_equal(back.astype(np.float32), pred.astype(np.float32))
    assert h["CRPIX1"] == (2 * (200.5 + 6) + 0.5 if upscale == 2 else 200.5 + 6) and h["IMG_FILE"] == "P0001_detxy.fits"
    assert os.path.exists(os.path.join(tmp_path, "out", "P0001_detxy_input.fits.gz"))


def test_repack_copies_empty_batch_and_inference_mode():
    cfg = dict(img_size=16, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=4, upscale=2,
               upsampler="pixelshuffledirect", resi_connection="3conv")
    state = gi.make_state(cfg, 11)
    m = _module(cfg, state)
    x = torch.from_numpy(gi.make_input((1, 1, 14, 15), 12)).cuda()

    def restated(sd):
        return si.swinir_forward({k: v.detach().cuda().double() if v.is_floating_point() else v.cuda() for k, v in sd.items()},
                                 x.double(), **cfg).float()

    y = m(x)                                       # grad mode on, parameters require grad: a graph node that refuses backward
    assert y.requires_grad and y.shape == (1, 1, 28, 30)
    with pytest.raises(RuntimeError, match="SwinIR training is not on the MI355X engine"):
        y.sum().backward()
    assert m(torch.zeros(0, 1, 14, 15, device="cuda")).shape == (0, 1, 28, 30)
    with torch.inference_mode():
        yi = m(x)
    with torch.no_grad():
        y0 = m(x)
        assert torch.equal(yi, y0) and torch.equal(y0, y.detach())
        twin = copy.deepcopy(m)                     # a used module: the copy builds its own engine and flat buffer
        clone = pickle.loads(pickle.dumps(m))
        m.layers[0].residual_group.blocks[1].attn.qkv.weight.mul_(0.5)     # in-place updates (what an optimizer step does): re-packed
        m.layers[0].conv[2].bias.add_(0.1)
        m.upsample[0].weight.mul_(1.5)
        m.layers[0].residual_group.blocks[0].attn.relative_position_bias_table.add_(0.3)
        y1 = m(x)
        assert not torch.equal(y1, y0)
        assert (y1 - restated(m.state_dict())).abs().max() < 1e-5
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
        assert torch.equal(m(x), y0)
        assert torch.equal(twin(x), y0) and torch.equal(clone.cuda()(x), y0)


def test_engine_refusals_name_their_argument():
    from xmm_superres_denoise.engine import SwinIREngine, XsdError

    def eng(**kw):
        a = dict(img_size=(32, 32), patch_size=(1, 1), in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=8, mlp_ratio=2.0,
                 qkv_bias=True, qk_scale=None, ape=False, patch_norm=True, upscale=1, img_range=1.0, upsampler="", resi_connection="1conv")
        a.update(kw)
        return SwinIREngine(**a)

    with pytest.raises(XsdError, match="ape=True"):
        eng(ape=True)
    with pytest.raises(XsdError, match="effective window of 24"):
        eng(img_size=(64, 64), window_size=24)
    with pytest.raises(XsdError, match="head dim 48"):
        eng(embed_dim=96)
    with pytest.raises(XsdError, match="3conv.*embed_dim >= 4"):
        eng(embed_dim=2, num_heads=[1], resi_connection="3conv")
    for up in (1, 3, 8):
        with pytest.raises(XsdError, match="nearest\\+conv.*upscale 2 or 4"):
            eng(upsampler="nearest+conv", upscale=up)
    for up in (0, 5, 16):
        with pytest.raises(XsdError, match=f"upscale {up} is not supported"):
            eng(upscale=up)
    with pytest.raises(XsdError, match="resi_connection"):
        eng(resi_connection="SFB")
    e = eng()
    assert e.L.xsd_swinir_set_math(e.h, 4) != 0 and b"f16x3" in e.L.xsd_last_error() and e.get_math() == "fp32"
    flat = torch.zeros(e.nparams, device="cuda")
    x = torch.zeros(1, 1, 16, 16, device="cuda")
    with pytest.raises(XsdError, match="pack_weights must be called"):
        e.forward(x)
    e.pack(flat)
    assert e.forward(x).shape == (1, 1, 16, 16)
    y = torch.empty(1, 1, 16, 16, device="cuda")
    for H, W in ((4, 16), (16, 3)):                           # pad 4 of 4 rows; pad 5 of 3 columns: F.pad's reflect raises there
        assert e.L.xsd_swinir_forward(e.h, x.data_ptr(), y.data_ptr(), 1, H, W, None) != 0
        assert b"reflect pad" in e.L.xsd_last_error() and f"H = {H}, W = {W}".encode() in e.L.xsd_last_error()
        with pytest.raises(XsdError, match="reflect pad"):
            e.out_size(H, W)
    g = eng(img_size=(20, 20), patch_size=(2, 2), window_size=12)              # effective window 10; the pads go to multiples of 12
    g.pack(torch.zeros(g.nparams, device="cuda"))
    with pytest.raises(XsdError, match="window_size 12.*effective window 10"):
        g.forward(torch.zeros(1, 1, 24, 24, device="cuda"))
    assert g.forward(torch.zeros(1, 1, 55, 60, device="cuda")).shape == (1, 1, 55, 60)
    # a workspace that cannot fit (about 0.6 TiB) is refused before anything is enqueued, and the engine stays usable
    big = eng(embed_dim=180, num_heads=[6])
    big.pack(torch.zeros(big.nparams, device="cuda"))
    xb, yb = torch.empty(64, 1, 1024, 1024, device="cuda"), torch.empty(1, device="cuda")
    assert big.L.xsd_swinir_forward(big.h, xb.data_ptr(), yb.data_ptr(), 64, 1024, 1024, None) == -4      # XSD_ERR_NOMEM
    assert b"workspace" in big.L.xsd_last_error()
    assert big.forward(x).shape == (1, 1, 16, 16)


def test_module_refusals_at_forward():
    from xmm_superres_denoise.engine import XsdError
    cfg = dict(img_size=32, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=8, upscale=1, upsampler="")
    m = _module(cfg, gi.make_state(cfg, 9))
    with pytest.raises(XsdError, match="reflect pad"):
        m(torch.zeros(1, 1, 4, 16, device="cuda"))
    with pytest.raises(XsdError, match=r"\[B,1,H,W\]"):
        m(torch.zeros(1, 3, 16, 16, device="cuda"))
    assert m(torch.zeros(1, 1, 9, 15, device="cuda")).shape == (1, 1, 9, 15)      # pad 7 of 9: the largest legal pad
