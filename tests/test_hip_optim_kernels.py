"""adam_kernel, l1_loss_kernel + l1_loss_final_kernel and clamp_bwd_kernel (csrc/aux_kernels.hip) one by one, through xsd_adam_step (no
engine), xsd_l1_loss and xsd_test_clamp_bwd.

Adam: torch.optim.Adam on the CPU in float64 is the reference and the same in float32 the yardstick (independent of oracle/xsd_oracle.c).
Per tensor (p, m, v each):  max|got - ref64| <= max(2 max|ref32 - ref64|, 6e-8 max|ref64|); the floor is one fp32 rounding.  The
references get lr, betas and eps as the C ABI carries them, i.e. rounded to float (hyper()): beta2 = 0.999f is 0.99900001287, so its
1 - beta2 differs from 0.001 by 1.3e-5 of itself, and a reference on the Python doubles would be another optimiser's `v`.
L1: the value against float64 (2e-6 max(1, |v|), the bar of tests/test_hip_loss.py), the gradient on the bits.  clamp_bwd: on the bits.
Every tensor of a launch lies between NaN guard bands in one allocation; read-only tensors must come back bit for bit."""
import numpy as np
import pytest
import torch

from util_hip import Guarded

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float32).tiny
CAP = 4096 * 256            # the grid cap of the elementwise launches: one element more needs a second pass of the grid-stride loop
SIZES = [1, 255, 256, 257, 100003, CAP + 77]
DEFAULT = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
CONFIGS = {
    "default": dict(),
    "betas": dict(betas=(0.5, 0.9)),
    "eps": dict(eps=1e-3),
    "lr": dict(lr=1e-3),
    "resumed": dict(step0=1000),
}
WORST = {}


@pytest.fixture(scope="module")
def L():
    from xmm_superres_denoise.engine import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(v):
    return float(np.float32(v))


def hyper(cfg):
    """lr, (beta1, beta2), eps as the floats xsd_adam_step receives"""
    c = {**DEFAULT, **{k: v for k, v in cfg.items() if k in DEFAULT}}
    return f32(c["lr"]), (f32(c["betas"][0]), f32(c["betas"][1])), f32(c["eps"])


def torch_adam(p0, m0, v0, grads, step0, lr, betas, eps, dtype):
    p = torch.from_numpy(p0).to(dtype).clone().requires_grad_(True)      # a copy: .to(float32) would alias p0 and the step would write it
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": torch.from_numpy(m0).to(dtype).clone(),
                    "exp_avg_sq": torch.from_numpy(v0).to(dtype).clone()}
    for g in grads:
        p.grad = torch.from_numpy(g).to(dtype)
        opt.step()
    st = opt.state[p]
    return [a.detach().numpy().astype(np.float64) for a in (p, st["exp_avg"], st["exp_avg_sq"])]


def hip_adam(L, p0, m0, v0, grads, step0, lr, betas, eps, grad_scale=1.0):
    """the steps on the device; every launch between guard bands, the gradient read-only"""
    g = Guarded(ro=("g",), p=p0, g=grads[0], m=m0, v=v0)
    for k, gr in enumerate(grads):
        if k:
            g.t["g"].copy_(torch.from_numpy(gr))
            g.before["g"] = g.t["g"].clone()
        rc = L.xsd_adam_step(None, g.ptr("p"), g.ptr("g"), g.ptr("m"), g.ptr("v"), p0.size, step0 + k, lr, betas[0], betas[1], eps, grad_scale, None)
        assert rc == 0, (rc, L.xsd_last_error().decode())
    torch.cuda.synchronize()
    g.check()
    return [g.np(k) for k in ("p", "m", "v")]


def hold(got, ref64, ref32, case):
    for name, a, r64, r32 in zip("pmv", got, ref64, ref32):
        err, yard, floor = np.abs(a - r64).max(), 2 * np.abs(r32 - r64).max(), 6e-8 * np.abs(r64).max()
        bar = max(yard, floor)
        ratio = err / bar if bar > 0 else 0.0
        key = (case.split("-")[0], name)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print(f"adam {case} {name}: max|got - ref64| {err:.3e}, 2 max|ref32 - ref64| {yard:.3e}, floor {floor:.3e}: {ratio:.2f} of the bar "
              f"(worst {key[0]} {name} so far {WORST[key]:.2f})")
        same = float((a.astype(np.float64) == r32).mean())       # reported, not asserted: torch's CPU kernels may round differently elsewhere
        print(f"adam {case} {name}: equal to torch's float32 result on the bits in {100 * same:.2f} % of the elements")
        assert err <= bar, f"{case} {name}: {err:.3e} > {bar:.3e}"


def start(n, seed, resumed=False):
    rng = np.random.default_rng(seed)
    p0 = (0.05 * rng.standard_normal(n)).astype(np.float32)
    m0 = (1e-3 * rng.standard_normal(n)).astype(np.float32) if resumed else np.zeros(n, np.float32)
    v0 = (1e-6 * rng.random(n)).astype(np.float32) if resumed else np.zeros(n, np.float32)
    return rng, p0, m0, v0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_adam_runs(L, config, n):
    """50 steps of fresh gradients; p, m and v each against float64, torch's float32 the yardstick.  On ONE element that yardstick is a
    single draw of torch's own rounding: the check holds there because adam_kernel performs torch's float operations in torch's order
    (csrc/aux_kernels.hip), so its m and v are torch's float32 values on the bits.  With the operation order left to the compiler's FMA
    contraction, v differed in its last bit and three of the fifteen one-element checks missed."""
    cfg = CONFIGS[config]
    step0 = cfg.get("step0", 1)
    lr, betas, eps = hyper(cfg)
    rng, p0, m0, v0 = start(n, 1000 + n % 9973, resumed=step0 > 1)
    grads = [(1e-3 * rng.standard_normal(n) * (1 + k % 3)).astype(np.float32) for k in range(50)]
    got = hip_adam(L, p0, m0, v0, grads, step0, lr, betas, eps)
    ref64 = torch_adam(p0, m0, v0, grads, step0, lr, betas, eps, torch.float64)
    ref32 = torch_adam(p0, m0, v0, grads, step0, lr, betas, eps, torch.float32)
    hold(got, ref64, ref32, f"{config}-n{n}")


def test_adam_single_step_late(L):
    """step = 100000: both bias corrections are within rounding of 1 (beta2^step = 3.5e-44)"""
    n = 100003
    lr, betas, eps = hyper({})
    rng, p0, m0, v0 = start(n, 7, resumed=True)
    grads = [(1e-3 * rng.standard_normal(n)).astype(np.float32)]
    got = hip_adam(L, p0, m0, v0, grads, 100000, lr, betas, eps)
    hold(got, torch_adam(p0, m0, v0, grads, 100000, lr, betas, eps, torch.float64),
         torch_adam(p0, m0, v0, grads, 100000, lr, betas, eps, torch.float32), "late-step100000")


@pytest.mark.parametrize("n", [257, CAP + 77])
def test_adam_grad_scale_is_a_premultiplied_gradient(L, n):
    """grad_scale = 0.25 (the data-parallel mean over 4 ranks; a power of two: the product is exact) == a step on 0.25 g, bit for bit,
    and both against float64"""
    lr, betas, eps = hyper({})
    rng, p0, m0, v0 = start(n, 8, resumed=True)
    g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    a = hip_adam(L, p0, m0, v0, [g], 3, lr, betas, eps, grad_scale=0.25)
    b = hip_adam(L, p0, m0, v0, [np.float32(0.25) * g], 3, lr, betas, eps)
    for x, y, name in zip(a, b, "pmv"):
        assert np.array_equal(bits(x), bits(y)), name
    one = hip_adam(L, p0, m0, v0, [g], 3, lr, betas, eps)
    assert not np.array_equal(bits(a[0]), bits(one[0])) and not np.array_equal(bits(a[2]), bits(one[2])), "grad_scale did nothing"
    hold(a, torch_adam(p0, m0, v0, [np.float32(0.25) * g], 3, lr, betas, eps, torch.float64),
         torch_adam(p0, m0, v0, [np.float32(0.25) * g], 3, lr, betas, eps, torch.float32), f"gscale-n{n}")


def test_adam_zero_gradient(L):
    """from zero state an all-zero gradient leaves p bit for bit (0 / eps = 0; -0.0 and subnormals included) and m = v = 0; after ten real
    steps a zero gradient still moves p (m decays, it does not vanish): against float64"""
    n = 1000
    lr, betas, eps = hyper({})
    rng, p0, m0, v0 = start(n, 9)
    p0[:4] = np.array([-0.0, 0.0, 1e-45, -TINY], np.float32)
    z = np.zeros(n, np.float32)
    got = hip_adam(L, p0, m0, v0, [z], 1, lr, betas, eps)
    assert np.array_equal(bits(got[0]), bits(p0)) and not got[1].any() and not got[2].any()
    grads = [(1e-3 * rng.standard_normal(n)).astype(np.float32) for _ in range(10)] + [z]
    got = hip_adam(L, p0, m0, v0, grads, 1, lr, betas, eps)
    ref64 = torch_adam(p0, m0, v0, grads, 1, lr, betas, eps, torch.float64)
    before = torch_adam(p0, m0, v0, grads[:10], 1, lr, betas, eps, torch.float64)
    assert np.median(np.abs(ref64[0] - before[0])) > 1e-5                  # the eleventh step still moves the parameters
    hold(got, ref64, torch_adam(p0, m0, v0, grads, 1, lr, betas, eps, torch.float32), "zero-after10")


@pytest.mark.parametrize("mag", [1e18, 1e-30])
def test_adam_extreme_gradients(L, mag):
    """|g| = 1e18: g^2 = 1e36 is still a float and the step is lr sign(g); |g| = 1e-30: g^2 underflows, v = 0 and the step is lr m / eps"""
    n = 257
    lr, betas, eps = hyper({})
    rng, p0, m0, v0 = start(n, 10)
    g = (mag * np.sign(rng.standard_normal(n)) * (1 + rng.random(n))).astype(np.float32)
    got = hip_adam(L, p0, m0, v0, [g], 1, lr, betas, eps)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    ref64 = torch_adam(p0, m0, v0, [g], 1, lr, betas, eps, torch.float64)
    if mag > 1:
        assert np.abs(np.abs(ref64[0] - p0) - lr).max() < 1e-3 * lr
    hold(got, ref64, torch_adam(p0, m0, v0, [g], 1, lr, betas, eps, torch.float32), f"extreme-{mag:g}")


def test_adam_is_deterministic(L):
    n = CAP + 77
    lr, betas, eps = hyper({})
    rng, p0, m0, v0 = start(n, 11, resumed=True)
    grads = [(1e-3 * rng.standard_normal(n)).astype(np.float32) for _ in range(2)]
    a = hip_adam(L, p0, m0, v0, grads, 5, lr, betas, eps)
    b = hip_adam(L, p0, m0, v0, grads, 5, lr, betas, eps)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


def test_adam_refusals_write_nothing(L):
    n = 300
    rng, p0, m0, v0 = start(n, 12, resumed=True)
    g = Guarded(ro=("p", "g", "m", "v"), p=p0, g=p0[::-1].copy(), m=m0, v=v0)
    ok = dict(p=g.ptr("p"), g=g.ptr("g"), m=g.ptr("m"), v=g.ptr("v"), n=n, step=1)
    for bad in (dict(n=0), dict(n=-5), dict(step=0), dict(step=-1), dict(p=None), dict(g=None), dict(m=None), dict(v=None)):
        a = {**ok, **bad}
        rc = L.xsd_adam_step(None, a["p"], a["g"], a["m"], a["v"], a["n"], a["step"], 2e-4, 0.9, 0.999, 1e-8, 1.0, None)
        assert rc < 0, bad
    torch.cuda.synchronize()
    g.check()


# =====================================================================================================================================
# mean-L1 loss
# =====================================================================================================================================

@pytest.fixture(scope="module")
def eng():
    from xmm_superres_denoise.engine import Engine
    return Engine("dn", 1, 1, 32, 1)


def l1_pair(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.random(n).astype(np.float32)
    y = np.clip(t + 0.1 * rng.standard_normal(n), 0, 1).astype(np.float32)
    eq = np.arange(n) % 3 == 0                      # y == t on a third of the elements ...
    y[eq] = t[eq]
    z = np.nonzero(eq)[0][::2]
    y[z], t[z] = 0.0, -0.0                          # ... half of them +0.0 against -0.0
    return y, t, eq


@pytest.mark.parametrize("want_dy", [True, False])
@pytest.mark.parametrize("n", [1, 257, 100003])
def test_l1(eng, n, want_dy):
    """value against float64; gradient exactly 0 where y == t (+0.0 against -0.0 included) and +-float32(1 / n) elsewhere; dy may be null"""
    y, t, eq = l1_pair(n, 50 + n % 97)
    if n == 1:
        y[0], t[0], eq[0] = 0.25, 0.75, False
    g = Guarded(ro=("y", "t"), y=y, t=t, dy=(n,), loss=(1,))
    rc = eng.L.xsd_l1_loss(eng.h, g.ptr("y"), g.ptr("t"), g.ptr("dy") if want_dy else None, g.ptr("loss"), n, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, eng.L.xsd_last_error().decode())
    g.check(untouched=() if want_dy else ("dy",))
    d = y.astype(np.float64) - t.astype(np.float64)
    v = np.abs(d).sum() / n
    got = float(g.np("loss")[0])
    print(f"l1 n {n}: value {got:.9g} (float64 {v:.9g}), {abs(got - v) / (2e-6 * max(1.0, abs(v))):.3f} of the bar")
    assert abs(got - v) <= 2e-6 * max(1.0, abs(v))
    if want_dy:
        inv = np.float32(1.0) / np.float32(n)
        want = np.where(d > 0, inv, np.where(d < 0, -inv, np.float32(0.0))).astype(np.float32)
        assert not want[eq].any() and np.array_equal(bits(g.np("dy")), bits(want))


def test_l1_nan_in_nan_out(eng):
    n = 100003
    y, t, _ = l1_pair(n, 60)
    y[n - 5] = np.nan
    g = Guarded(ro=("y", "t"), y=y, t=t, dy=(n,), loss=(1,))
    rc = eng.L.xsd_l1_loss(eng.h, g.ptr("y"), g.ptr("t"), g.ptr("dy"), g.ptr("loss"), n, None)
    torch.cuda.synchronize()
    assert rc == 0
    g.check()
    assert np.isnan(g.np("loss")[0])
    dy = g.np("dy")
    assert dy[n - 5] == 0 and np.isfinite(dy).all()      # sign(NaN) takes neither branch; every other element is untouched by it


# =====================================================================================================================================
# clamp backward of the plane path
# =====================================================================================================================================

def clamp_bwd(L, pre, dy):
    g = Guarded(ro=("pre", "dy"), pre=pre, dy=dy, d=(pre.size,))
    rc = L.xsd_test_clamp_bwd(g.ptr("pre"), g.ptr("dy"), g.ptr("d"), pre.size, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.xsd_last_error().decode())
    g.check()
    return g.np("d")


def test_clamp_bwd_at_the_bounds(L):
    """the gradient passes iff 0 <= pre <= 1 (bounds included, like torch.clamp); NaN and +-inf block it"""
    pre = np.array([-TINY, -0.0, 0.0, 1e-45, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf, -np.inf, np.nan], np.float32)
    passes = np.array([0, 1, 1, 1, 1, 1, 0, 0, 0, 0], bool)
    n = 70
    pre, passes = np.resize(pre, n), np.resize(passes, n)
    dy = np.random.default_rng(70).normal(size=n).astype(np.float32)
    want = np.where(passes, dy, np.float32(0.0))
    assert np.array_equal(bits(clamp_bwd(L, pre, dy)), bits(want))
    x = torch.from_numpy(np.nan_to_num(pre, nan=2.0)).double().requires_grad_(True)      # torch agrees on every non-NaN entry
    tg, = torch.autograd.grad(x.clamp(0, 1), x, torch.from_numpy(dy).double())
    assert np.array_equal(tg.numpy().astype(np.float32), want)


def test_clamp_bwd_second_pass(L):
    n = CAP + 77
    rng = np.random.default_rng(71)
    pre = rng.normal(0.5, 0.6, size=n).astype(np.float32)
    dy = rng.normal(size=n).astype(np.float32)
    want = np.where((pre >= 0) & (pre <= 1), dy, np.float32(0.0))
    assert np.array_equal(bits(clamp_bwd(L, pre, dy)), bits(want))


def test_clamp_bwd_refusals(L):
    g = Guarded(ro=("a", "b", "c"), a=np.ones(8, np.float32), b=np.ones(8, np.float32), c=np.ones(8, np.float32))
    assert L.xsd_test_clamp_bwd(g.ptr("a"), g.ptr("b"), g.ptr("c"), 0, None) < 0
    assert L.xsd_test_clamp_bwd(None, g.ptr("b"), g.ptr("c"), 8, None) < 0
    assert L.xsd_test_clamp_bwd(g.ptr("a"), None, g.ptr("c"), 8, None) < 0
    assert L.xsd_test_clamp_bwd(g.ptr("a"), g.ptr("b"), None, 8, None) < 0
    torch.cuda.synchronize()
    g.check()
