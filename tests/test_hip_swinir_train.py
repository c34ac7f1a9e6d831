"""TrainableSwinIR (models/modules/swinir_train.py) and train.fit_swinir: the SwinIR forward composed of the differentiable HIP ops, its
gradients through torch's autograd, Adam steps, DropPath and the checkpoint round trip, against the float64 run of the plain-torch
restatement tests/golden/swinir_torch.py.  The bar is test_hip_sw_kernels._assert_within_2x_of_fp32 with a non-zero yardstick, as in
test_hip_sw_ops.py.  Every model test runs with drop_path_rate = 0 except the DropPath tests themselves."""
import copy
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_swinir as gi
import swinfir_torch as st
import swinir_torch as sit
from test_hip_sw_kernels import _assert_within_2x_of_fp32

pytestmark = pytest.mark.gpu

DN = dict(img_size=64, patch_size=1, in_chans=1, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=4, upscale=1, upsampler="",
          drop_path_rate=0.0)
SR = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=12, depths=[2, 2], num_heads=[2, 2], window_size=4, upscale=2,
          upsampler="pixelshuffle", qkv_bias=False, drop_path_rate=0.0)


def _bar(y, y32, y64, what):
    rms32 = _assert_within_2x_of_fp32(y, y32, y64, what)
    assert rms32 > 0, (what, "the fp32 yardstick is exact here")
    return rms32


def _build(cfg, seed, **kw):
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    state = gi.make_state(cfg, seed)
    m = SwinIR(**gi.full_cfg(**cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return TrainableSwinIR(m.cuda(), **kw)


def _sd(module, dtype, grad=False):
    """the wrapped module's state dict in `dtype`: the parameters as leaves (requiring a gradient with `grad`), the buffers as they are"""
    names = {k for k, _ in module.named_parameters()}
    return OrderedDict((k, v.detach().to(dtype, copy=True).requires_grad_(grad) if k in names else v.detach()) for k, v in module.state_dict().items())


def _ref_grads(module, cfg, x, dy, dtype):
    sd = _sd(module, dtype, True)
    xl = x.to(dtype).detach().requires_grad_(True)
    y = sit.swinir_forward(sd, xl, **cfg)
    y.backward(dy.to(dtype))
    return y.detach(), xl.grad, {k: v.grad for k, v in sd.items() if v.requires_grad}


@pytest.mark.parametrize("name,cfg,shape", [("denoiser", DN, (2, 1, 18, 21)), ("x2 pixelshuffle", SR, (1, 3, 8, 12))])
def test_output_and_every_gradient_against_float64(name, cfg, shape):
    net = _build(cfg, 401).train()
    x = torch.from_numpy(gi.make_input(shape, 402)).cuda().requires_grad_(True)
    y = net(x)
    up = cfg["upscale"]
    assert y.shape == (shape[0], shape[1], shape[2] * up, shape[3] * up)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(403)).cuda()
    y.backward(dy)
    y64, dx64, g64 = _ref_grads(net.module, cfg, x, dy, torch.float64)
    y32, dx32, g32 = _ref_grads(net.module, cfg, x, dy, torch.float32)
    _bar(y, y32, y64, f"{name}: output")
    _bar(x.grad, dx32, dx64, f"{name}: d input")
    named = dict(net.module.named_parameters())
    assert set(named) == set(g64) and all(p.grad is not None for p in named.values())
    failed = []
    for k, p in named.items():
        try:
            _bar(p.grad, g32[k], g64[k], f"{name}: d {k}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def test_trainable_and_fused_forward_before_and_after_training():
    """in eval the composed forward and the wrapped module's fused engine forward both meet the bar; after Adam steps the fused forward has
    re-packed: it sees the trained weights"""
    net = _build(DN, 411)
    x = torch.from_numpy(gi.make_input((2, 1, 18, 21), 412)).cuda()
    target = torch.from_numpy(gi.make_input((2, 1, 18, 21), 413)).cuda()

    def check(what):
        net.eval()
        with torch.no_grad():
            yt, yf = net(x), net.module(x)
            y64 = sit.swinir_forward(_sd(net.module, torch.float64), x.double(), **DN)
            y32 = sit.swinir_forward(_sd(net.module, torch.float32), x, **DN)
        _bar(yt, y32, y64, f"{what}: trainable forward")
        _bar(yf, y32, y64, f"{what}: fused forward")
        return yf
    before = check("before training")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for _ in range(3):
        net.train()
        opt.zero_grad()
        F.l1_loss(net(x), target).backward()
        opt.step()
    after = check("after 3 Adam steps")
    assert not torch.equal(before, after)


def test_five_adam_steps_follow_the_float64_trajectory():
    from xmm_superres_denoise.train import SwinIRTrainer
    net = _build(DN, 421)
    x = torch.from_numpy(gi.make_input((2, 1, 18, 21), 422)).cuda()
    target = torch.from_numpy(gi.make_input((2, 1, 18, 21), 423)).cuda()
    lr = 1e-3
    runs = {}
    for dtype in (torch.float64, torch.float32):
        sd = _sd(net.module, dtype, True)
        params = [v for v in sd.values() if v.requires_grad]
        opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = F.l1_loss(sit.swinir_forward(sd, x.to(dtype), **DN), target.to(dtype))
            loss.backward()
            opt.step()
            losses.append(float(loss))
        runs[dtype] = (torch.cat([p.detach().reshape(-1).double() for p in params]), losses)
    trainer = SwinIRTrainer(net, lr=lr, betas=(0.9, 0.999))
    losses = [float(trainer.train_step(x, target)) for _ in range(5)]
    mine = torch.cat([p.detach().reshape(-1).double() for p in net.module.parameters()])
    ref, l64 = runs[torch.float64]
    p32, l32 = runs[torch.float32]
    rms = float((mine - ref).pow(2).mean().sqrt())
    rms32 = float((p32 - ref).pow(2).mean().sqrt())
    print(f"loss float64 {l64}\nloss fp32    {l32}\nloss engine  {losses}")
    print(f"parameters after 5 Adam steps: engine rms {rms:.3e} | fp32 torch rms {rms32:.3e} (ratio {rms / rms32:.3f})")
    assert trainer.step_count == 5 and rms32 > 0 and rms <= 2 * rms32, (rms, rms32)


def _forward_with_masks(sd, x, cfg, masks, dpr):
    """swinir_torch.swinir_forward's denoising path from swinfir_torch's pieces, each residual branch of block k scaled by
    mask / (1 - dpr[k]) per sample (modules.py drop_path)"""
    c = gi.full_cfg(**cfg)
    E, w = c["embed_dim"], c["window_size"]
    ws, shift, _ = gi.window_of(cfg)
    H0, W0 = x.shape[2:]
    x = F.pad(x, (0, (w - W0 % w) % w, 0, (w - H0 % w) % w), "reflect") * c["img_range"]
    xf = st._conv(x, sd, "conv_first", 1)
    B, _, H, W = xf.shape
    t = st._ln(xf.flatten(2).transpose(1, 2), sd, "patch_embed.norm")
    k, it = 0, iter(masks)
    for i, (depth, heads) in enumerate(zip(c["depths"], c["num_heads"])):
        scale = (E // heads) ** -0.5
        t0 = t
        for j in range(depth):
            p = f"layers.{i}.residual_group.blocks.{j}."
            o = st.window_attention(st._lin(st._ln(t, sd, p + "norm1"), sd, p + "attn.qkv"), sd[p + "attn.relative_position_bias_table"], H, W,
                                    heads, ws, shift if j % 2 else 0, scale)
            t = t + st._lin(o, sd, p + "attn.proj") / (1 - dpr[k]) * next(it).to(t.dtype).view(B, 1, 1)
            h = st._lin(F.gelu(st._lin(st._ln(t, sd, p + "norm2"), sd, p + "mlp.fc1")), sd, p + "mlp.fc2")
            t = t + h / (1 - dpr[k]) * next(it).to(t.dtype).view(B, 1, 1)
            k += 1
        t = st._conv(t.transpose(1, 2).reshape(B, E, H, W), sd, f"layers.{i}.conv", 1).flatten(2).transpose(1, 2) + t0
    img = st._ln(t, sd, "norm").transpose(1, 2).reshape(B, E, H, W)
    img = st._conv(img, sd, "conv_after_body", 1) + xf
    y = (x + st._conv(img, sd, "conv_last", 1)) / c["img_range"]
    return y[:, :, :H0, :W0]


def test_drop_path():
    from xmm_superres_denoise.models.modules.swinir_train import drop_path_schedule
    x = torch.from_numpy(gi.make_input((4, 1, 18, 21), 432)).cuda()
    net = _build(DN, 431)
    with torch.no_grad():
        assert torch.equal(net.train()(x), net.eval()(x)) and net.last_drop_masks == []            # rate 0: train() is eval()
        y_eval = net.eval()(x)
    y_graph = net.train()(x)                                                                       # with a graph: the activations run split
    assert y_graph.requires_grad and torch.equal(y_graph.detach(), y_eval)
    net = _build(DN, 431, drop_path_rate=0.5, generator=torch.Generator(device="cuda").manual_seed(7))
    dpr = drop_path_schedule(DN["depths"], 0.5)
    assert net.drop_path == dpr and dpr[0] == 0.0 and abs(dpr[-1] - 0.5) < 1e-7
    with torch.no_grad():
        y_eval = net.eval()(x)
        assert net.last_drop_masks == []
        y = net.train()(x)
    masks = net.last_drop_masks
    assert len(masks) == 2 * sum(DN["depths"]) and all(m.shape == (4,) and set(m.tolist()) <= {0.0, 1.0} for m in masks)
    assert torch.all(masks[0] == 1) and torch.all(masks[1] == 1)                                   # the first block keeps every sample
    assert any(float(m.min()) == 0.0 for m in masks) and not torch.equal(y, y_eval)
    y64 = _forward_with_masks(_sd(net.module, torch.float64), x.double(), DN, masks, dpr)
    y32 = _forward_with_masks(_sd(net.module, torch.float32), x, DN, masks, dpr)
    _bar(y, y32, y64, "drop path 0.5 with the recorded masks")
    # the same seed draws the same masks
    again = _build(DN, 431, drop_path_rate=0.5, generator=torch.Generator(device="cuda").manual_seed(7)).train()
    with torch.no_grad():
        assert torch.equal(again(x), y)


def test_fit_swinir_checkpoint_round_trip(tmp_path):
    from xmm_superres_denoise.infer import infer_file, load_swinir, write_fits
    from xmm_superres_denoise.train import SwinIRTrainer, fit_swinir, load_checkpoint
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    ctor = dict(img_size=64, patch_size=1, in_chans=1, embed_dim=16, depths=[2], num_heads=[2], window_size=8, upscale=1, upsampler="",
                drop_path_rate=0.0)
    ck = os.path.join(tmp_path, "swinir_fit.ckpt")
    net, trainer, losses = fit_swinir(ctor, steps=3, batch_size=2, lr_res=24, lr=1e-3, seed=3, checkpoint=ck, log_every=0)
    assert len(losses) == 3 and all(np.isfinite(losses)) and trainer.step_count == 3 and not net.training
    raw = torch.load(ck, map_location="cpu", weights_only=True)
    assert list(raw["state_dict"]) == ["model." + k for k in gi.param_shapes(ctor)] and raw["adam"]["step"] == 3
    m = load_swinir(ck, **ctor)
    for (k, v), (k2, v2) in zip(m.state_dict().items(), net.state_dict().items()):
        assert k == k2 and torch.equal(v.cpu(), v2.cpu()), k
    fresh = SwinIRTrainer(TrainableSwinIR(SwinIR(**ctor).cuda()), lr=1e-3)
    load_checkpoint(ck, fresh, fresh)
    assert fresh.step_count == 3 and torch.equal(fresh.m, trainer.m) and torch.equal(fresh.v, trainer.v) and float(trainer.v.abs().sum()) > 0
    assert fresh.opt.state[fresh.params[0]]["exp_avg"].data_ptr() == fresh.m.data_ptr()
    # an iterable of (lr, hr) batches continues from the restored state exactly as the original trainer would
    g = torch.Generator().manual_seed(5)
    batch = (torch.rand(1, 1, 16, 16, generator=g).cuda(), torch.rand(1, 1, 16, 16, generator=g).cuda())
    assert float(fresh.train_step(*batch)) == float(trainer.train_step(*batch))
    assert all(torch.equal(p, q) for p, q in zip(fresh.model.parameters(), trainer.model.parameters()))
    counts = np.random.default_rng(5).poisson(0.3, size=(403, 411)).astype(np.float32)
    src = os.path.join(tmp_path, "P0001_detxy.fits")
    write_fits(src, counts, OrderedDict(CRPIX1=200.5, CRPIX2=204.5, CDELT1=-0.001, CDELT2=0.001, PA_PNT=12.5, EXPOSURE=10000.0))
    pred, out_path = infer_file(src, m, None, os.path.join(tmp_path, "out"))
    assert pred.shape == (416, 416) and np.isfinite(pred).all() and out_path.endswith("P0001_detxy_dn_predict.fits.gz")


def test_fit_swinir_takes_batches_a_composed_loss_and_the_clamp():
    from xmm_superres_denoise.train import fit_swinir
    from xmm_superres_denoise.utils import create_loss, load_loss_config
    g = torch.Generator().manual_seed(9)
    data = [(torch.rand(1, 1, 320, 320, generator=g).cuda(), torch.rand(1, 1, 320, 320, generator=g).cuda()) for _ in range(2)]
    ctor = dict(img_size=64, in_chans=1, embed_dim=8, depths=[1], num_heads=[1], window_size=8, upscale=1, upsampler="", drop_path_rate=0.0)
    net, trainer, losses = fit_swinir(ctor, steps=None, data=data, loss=create_loss(*load_loss_config("linear")), clamp=True, log_every=0)
    assert len(losses) == 2 and all(np.isfinite(losses)) and trainer.step_count == 2 and net.clamp
    with pytest.raises(ValueError, match="loss 'mse' is not supported"):
        fit_swinir(ctor, loss="mse")


def test_copies_pickles_and_refusals():
    from xmm_superres_denoise.models import SwinIR, TrainableSwinIR
    net = _build(DN, 441, drop_path_rate=0.25, generator=torch.Generator(device="cuda").manual_seed(1))
    x = torch.from_numpy(gi.make_input((1, 1, 8, 8), 442)).cuda()
    with torch.no_grad():
        y = net.eval()(x)
        for other in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
            assert other.generator is None and other.drop_path_rate == 0.25 and other.module is not net.module
            assert torch.equal(other.eval()(x), y) and torch.equal(other.module(x), net.module(x))
    assert list(net.state_dict()) == list(net.module.state_dict())
    assert {id(p) for p in net.parameters()} == {id(p) for p in net.module.parameters()}
    # a second differentiation is refused by name
    xl = x.clone().requires_grad_(True)
    wgt = torch.ones(1, 1, 8, 8, device="cuda", requires_grad=True)
    g, = torch.autograd.grad((net(xl) * wgt).sum(), xl, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # models.SwinIR keeps its refusal
    with pytest.raises(RuntimeError, match="SwinIR training is not on the MI355X engine"):
        net.module(xl).sum().backward()
