"""CPU checks of the extended test metrics (gmsd, ms_gmsd, haarpsi, msdi, vif_p): the plain-torch restatement
tests/golden/ext_metrics_torch.py -- this project's specification of them, restated from the published code of piq 0.7.x and
torchmetrics 1.x; PARITY WITH THE LIBRARIES THEMSELVES IS UNPINNED (neither is available here), as for psnr / ssim / ms_ssim --
against things that do not depend on it (identities, closed forms, explicit-loop numpy versions written out index by index,
scipy's correlations), the stored float64 values, and the host side of the collection: key names, the reference's epoch
reduction, the refusals."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import ext_metrics_torch as E
import make_golden_ext_metrics as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _pair(shape, seed):
    return E.photon_pair(shape, torch.Generator().manual_seed(seed))


# ---- identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 61, 53)])
def test_identical_images(shape):
    _, t = _pair(shape, 1)
    assert E.gmsd(t, t).abs().max() < 1e-12 and E.ms_gmsd(t, t).abs().max() < 1e-12
    assert (E.haarpsi(t, t) - 1).abs().max() < 1e-9         # v = sigmoid(alpha) -> logit(v) / alpha = 1
    # vif_p: with p = t every window has g = s / (s + 1e-10) (s = sigma_t^2) and sigma_v^2 = 1e-10, so per window
    # den - num = log10((1 + s/2) / (1 + g^2 s / (2 + 1e-10))) <= (s (1 - g^2) / 2 + 1e-10 s / 4) / ln 10 <= 1.1e-10 / ln 10  (s <= 1/4),
    # and 0 where s < 1e-10: the value is 1 up to those epsilons, 0 <= den - num <= 1.1e-10 * (number of windows) / ln 10
    num, den = E.vif_parts(t, t)
    h, w, windows = shape[1], shape[2], 0
    for s in range(4):
        n = 2 ** (4 - s) + 1
        if s:
            h, w = (h - n + 2) // 2, (w - n + 2) // 2
        windows += (h - n + 1) * (w - n + 1)
    assert ((den - num) >= -1e-13).all() and ((den - num) <= 1.1e-10 * windows / math.log(10)).all()
    assert (E.vif_p(t, t) - 1).abs().max() < 1e-6
    # msdi: the 0.25 power turns a 1e-16 deviation into 1e-4, so the deviation is what is tested, not its root
    assert E.mdsi_deviation(t, t).abs().max() < 1e-12


# ---- closed forms on linear ramps ------------------------------------------------------------------------------------
def test_ramps_closed_form():
    a, b, H, W = 0.004, 0.007, 12, 16
    col = torch.arange(W, dtype=F64)[None, None, None, :].expand(1, 1, H, W)
    x, y = a * col, b * col
    gx = E.prewitt_grad(x)[0, 0]
    # interior: three rows of (x[j+1] - x[j-1]) / 3 = 2a, nothing vertical
    assert torch.allclose(gx[1:-1, 1:-1], torch.full((H - 2, W - 2), 2 * a, dtype=F64), rtol=1e-13, atol=0)
    # top row, interior column j: the zero row above leaves 2 of 3 rows horizontally and (a(j-1) + aj + a(j+1)) / 3 = aj vertically
    j = 5
    assert abs(gx[0, j].item() - math.hypot(4 * a / 3, a * j)) < 1e-15
    # left column, interior row: the zero column at the left: 3 * a * 1 / 3 = a horizontally, nothing vertical
    assert abs(gx[4, 0].item() - a) < 1e-15
    # corner (0, 0): horizontal 2 rows * a / 3, vertical (0 + a) / 3
    assert abs(gx[0, 0].item() - math.hypot(2 * a / 3, a / 3)) < 1e-15
    # pool2 of the ramp a*j is the ramp a*(2j + 0.5): interior gradient 4a, so the GMSD map's interior is (2*4a*4b + t) / (16a^2 + 16b^2 + t)
    px, py = E.pool2(x), E.pool2(y)
    assert torch.allclose(px[0, 0, 0], a * (2 * torch.arange(W // 2, dtype=F64) + 0.5), rtol=1e-13)
    t = 170 / 255 ** 2
    g = E.sim(E.prewitt_grad(px), E.prewitt_grad(py), t)[0, 0, 1:-1, 1:-1]
    want = (2 * 4 * a * 4 * b + t) / (16 * a * a + 16 * b * b + t)
    assert torch.allclose(g, torch.full_like(g, want), rtol=1e-13, atol=0)
    # MS-GMSD, scale 0, interior: gradients 255 * 2a and 255 * 2b, alpha = 0.5, t = 170
    A, B = 255 * 2 * a, 255 * 2 * b
    assert abs(((2 - 0.5) * A * B + 170) / (A * A + B * B - 0.5 * A * B + 170) - 0.99) < 0.01       # (a sanity range for the line below)
    s0 = E.ms_gmsd_scales(x[:, 0], y[:, 0])[0, 0].item()
    assert 0 < s0 < 0.05      # only the borders deviate from the interior's constant


# ---- explicit-loop versions on tiny images ---------------------------------------------------------------------------
def _np_pool2(x):
    H, W = x.shape
    d = max(H % 2, W % 2)
    p = np.zeros((H + d, W + d))
    p[:H, :W] = x
    return np.array([[(p[2 * i, 2 * j] + p[2 * i, 2 * j + 1] + p[2 * i + 1, 2 * j] + p[2 * i + 1, 2 * j + 1]) / 4
                      for j in range((W + d) // 2)] for i in range((H + d) // 2)])


def _np_grad(x):
    H, W = x.shape
    p = np.zeros((H + 2, W + 2))
    p[1:-1, 1:-1] = x
    g = np.zeros((H, W))
    for i in range(H):
        for j in range(W):
            n = p[i:i + 3, j:j + 3]
            gx = (n[:, 2].sum() - n[:, 0].sum()) / 3
            gy = (n[2, :].sum() - n[0, :].sum()) / 3
            g[i, j] = math.hypot(gx, gy)
    return g


def _np_gmsd(x, y):
    a, b = _np_grad(_np_pool2(x)), _np_grad(_np_pool2(y))
    t = 170 / 255 ** 2
    return ((2 * a * b + t) / (a * a + b * b + t)).std()


def _np_ms_gmsd(x, y):
    x, y, tot = 255 * x, 255 * y, 0.0
    for k, w in enumerate((0.096, 0.596, 0.289, 0.019)):
        if k:
            x, y = _np_pool2(x), _np_pool2(y)
        a, b = _np_grad(x), _np_grad(y)
        tot += w * ((1.5 * a * b + 170) / (a * a + b * b - 0.5 * a * b + 170)).std() ** 2
    return math.sqrt(tot)


def _np_haar(x, s):
    """|coefficients| [2, H, W] of scale s by explicit sums: rows i - k/2 + 1 .. i + k/2, the upper half +1/k, the lower half -1/k"""
    H, W = x.shape
    k, out = 2 ** (s + 1), np.zeros((2, H, W))
    for i in range(H):
        for j in range(W):
            for dr in range(-(k // 2) + 1, k // 2 + 1):
                for dc in range(-(k // 2) + 1, k // 2 + 1):
                    r, c = i + dr, j + dc
                    v = x[r, c] / k if 0 <= r < H and 0 <= c < W else 0.0
                    out[0, i, j] += v if dr <= 0 else -v
                    out[1, i, j] += v if dc <= 0 else -v
    return np.abs(out)


def _np_haarpsi(x, y):
    x, y = _np_pool2(255 * x), _np_pool2(255 * y)
    cx, cy = [_np_haar(x, s) for s in range(3)], [_np_haar(y, s) for s in range(3)]
    w = np.maximum(cx[2], cy[2])
    sim = lambda a, b: (2 * a * b + 30) / (a * a + b * b + 30)      # noqa: E731
    s = (sim(cx[0], cy[0]) + sim(cx[1], cy[1])) / 2
    eps = 2.0 ** -23
    v = ((w / (1 + np.exp(-4.2 * s))).sum() + eps) / (w.sum() + eps)
    return (math.log(v / (1 - v)) / 4.2) ** 2


def _np_mdsi(x, y):      # min(H, W) < 384: k = 1, no pooling
    lx, ly = 0.9999 * 255 * x, 0.9999 * 255 * y
    gx, gy, ga = _np_grad(lx), _np_grad(ly), _np_grad((lx + ly) / 2)
    sim = lambda a, b, c: (2 * a * b + c) / (a * a + b * b + c)     # noqa: E731
    gs = sim(gx, gy, 140) + sim(gx, ga, 55) - sim(gy, ga, 55)
    hx, hy, mx, my = -0.01 * 255 * x, -0.01 * 255 * y, -0.09 * 255 * x, -0.09 * 255 * y
    cs = (2 * (hx * hy + mx * my) + 550) / (hx ** 2 + hy ** 2 + mx ** 2 + my ** 2 + 550)
    z = (0.6 * gs + 0.4 * cs).astype(complex) ** 0.25
    return np.abs(z - z.mean()).mean() ** 0.25


def _np_vif(p, t):
    num = den = 0.0
    for s in range(4):
        n = 2 ** (4 - s) + 1
        c = np.arange(n) - n // 2
        k = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2 * (n / 3) ** 2))
        k /= k.sum()

        def win(a, step=1):
            return np.array([[(a[i:i + n, j:j + n] * k).sum() for j in range(0, a.shape[1] - n + 1, step)]
                             for i in range(0, a.shape[0] - n + 1, step)])
        if s:
            t, p = win(t, 2), win(p, 2)
        mt, mp = win(t), win(p)
        st, sp, stp = np.maximum(win(t * t) - mt * mt, 0), np.maximum(win(p * p) - mp * mp, 0), win(t * p) - mt * mp
        for a, b, c_ in zip(st.ravel(), sp.ravel(), stp.ravel()):
            g = c_ / (a + 1e-10)
            sv = b - g * c_
            if a < 1e-10:
                g, sv, a = 0.0, b, 0.0
            if b < 1e-10:
                g, sv = 0.0, 0.0
            if g < 0:
                sv, g = b, 0.0
            sv = max(sv, 1e-10)
            num += math.log10(1 + g * g * a / (sv + 2))
            den += math.log10(1 + a / 2)
    return num / den


def test_explicit_loops_on_tiny_images():
    p, t = _pair((1, 12, 9), 2)
    x, y = p[0].numpy(), t[0].numpy()
    assert abs(E.gmsd(p, t).item() - _np_gmsd(x, y)) < 1e-13
    p, t = _pair((1, 19, 22), 3)
    x, y = p[0].numpy(), t[0].numpy()
    assert abs(E.ms_gmsd(p, t).item() - _np_ms_gmsd(x, y)) < 1e-13
    assert abs(E.haarpsi(p, t).item() - _np_haarpsi(x, y)) < 1e-11
    assert abs(E.msdi(p, t).item() - _np_mdsi(x, y)) < 1e-12
    p, t = _pair((1, 41, 43), 4)
    assert abs(E.vif_p(p, t).item() - _np_vif(p[0].numpy(), t[0].numpy())) < 1e-11


def test_mdsi_complex_power_of_a_negative_g():
    """G < 0 -> z = |G|^q (cos q pi, sin q pi), what Python's own complex power gives; G >= 0 stays real"""
    g = torch.tensor([-16.0, 81.0, 0.0, -1e-3], dtype=F64)
    re, im = E.complex_power(g, 0.25)
    for k, v in enumerate(g.tolist()):
        z = complex(v, 0.0) ** 0.25 if v else 0j
        assert abs(re[k].item() - z.real) < 1e-14 and abs(im[k].item() - z.imag) < 1e-14, (v, z)
    assert abs(re[0].item() - math.sqrt(2)) < 1e-14 and abs(im[0].item() - math.sqrt(2)) < 1e-14 and re[1].item() == 3 and im[1].item() == 0


# ---- stencils and poolings against scipy / numpy ---------------------------------------------------------------------
def test_stencils_against_scipy():
    from scipy import ndimage, signal
    p, _ = _pair((1, 37, 29), 5)
    x = p[0].numpy()
    k = np.array([[-1.0, 0.0, 1.0]] * 3) / 3
    want = np.hypot(ndimage.correlate(x, k, mode="constant"), ndimage.correlate(x, k.T, mode="constant"))
    assert np.abs(E.prewitt_grad(p[:, None])[0, 0].numpy() - want).max() < 1e-14
    for s in range(3):
        kk = 2 ** (s + 1)
        h = np.ones((kk, kk)) / kk
        h[kk // 2:] *= -1
        pad = np.pad(x, ((kk // 2 - 1, kk // 2), (kk // 2 - 1, kk // 2)))
        got = E.haar_coefficients(p[:, None], s)[0].numpy()
        assert got.shape == (2,) + x.shape
        assert np.abs(got[0] - signal.correlate2d(pad, h, mode="valid")).max() < 1e-13
        assert np.abs(got[1] - signal.correlate2d(pad, h.T, mode="valid")).max() < 1e-13
    for n in (17, 9, 5, 3):
        kn = E.vif_kernel(n, F64)[0, 0].numpy()
        assert abs(kn.sum() - 1) < 1e-14 and kn.shape == (n, n) and abs(kn[n // 2, n // 2 + 1] / kn[n // 2, n // 2] - math.exp(-4.5 / n ** 2)) < 1e-14
        got = torch.nn.functional.conv2d(p[:, None], E.vif_kernel(n, F64))[0, 0].numpy()
        assert np.abs(got - signal.correlate2d(x, kn, mode="valid")).max() < 1e-14


@pytest.mark.parametrize("shape", [(61, 53), (417, 403), (64, 33), (33, 64)])
def test_pool2_and_mdsi_pooling_on_odd_sizes(shape):
    H, W = shape
    x = torch.rand((1, 1, H, W), dtype=F64, generator=torch.Generator().manual_seed(H))
    d = max(H % 2, W % 2)
    got = E.pool2(x)[0, 0].numpy()
    assert got.shape == ((H + d) // 2, (W + d) // 2)
    pad = np.zeros((H + d + 1, W + d + 1))
    pad[:H, :W] = x[0, 0].numpy()
    h2, w2 = got.shape
    want = pad[:2 * h2, :2 * w2].reshape(h2, 2, w2, 2).mean((1, 3))
    assert np.abs(got - want).max() < 1e-15
    k = E.mdsi_kernel_size(H, W)
    assert k == {53: 1, 403: 2, 33: 1}[min(H, W)]
    got = E.mdsi_pool(x)[0, 0].numpy()
    mh, mw = (H - 1) // k + 1, (W - 1) // k + 1
    assert got.shape == (mh, mw)
    pad = np.zeros((mh * k + k, mw * k + k))
    pad[(k - 1) // 2:(k - 1) // 2 + H, (k - 1) // 2:(k - 1) // 2 + W] = x[0, 0].numpy()
    want = pad[:mh * k, :mw * k].reshape(mh, k, mw, k).mean((1, 3))
    assert np.abs(got - want).max() < 1e-15


def test_mdsi_kernel_size_rounds_like_python():
    assert [E.mdsi_kernel_size(n, 4096) for n in (41, 127, 128, 129, 383, 384, 385, 416, 640, 641, 832, 896)] == \
        [1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 4]          # 128 / 256 = 0.5 -> 0 -> max(1, .); 384 -> 1.5 -> 2; 640 -> 2.5 -> 2 (ties to even)


# ---- stored values ---------------------------------------------------------------------------------------------------
def test_restatement_has_not_drifted_from_the_stored_values():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ext_metrics_cases.npz"))
    seen = 0
    for name, (p, t) in mg.cases().items():
        assert np.allclose(z[name + "/checksum"], [p.sum().item(), t.sum().item()], rtol=1e-12), name      # the seeded inputs are the same
        for k, v in mg.values(p, t).items():
            assert np.allclose(v, z[f"{name}/{k}"], rtol=1e-9, atol=0), (name, k, v, z[f"{name}/{k}"])
            seen += 1
    assert seen == len(z.files) - len(mg.CASES)


def test_anchor_values_of_the_specification():
    """the float64 values the specification quotes for its own recipe (torch.manual_seed(0), B = 2, sizes drawn in the order
    416^2, 832^2, 61x53; first image of each batch), to ~6 digits"""
    import torch.nn.functional as Fn
    torch.manual_seed(0)
    pairs = []
    for shape in ((2, 416, 416), (2, 832, 832), (2, 61, 53)):
        t = torch.poisson(torch.full(shape, 0.3, dtype=F64))
        t = Fn.avg_pool2d(torch.clamp(t / 6, 0, 1)[:, None], 3, 1, 1)[:, 0]
        pairs.append((torch.clamp(t + 0.05 * torch.randn_like(t), 0, 1), t))
    want = {0: dict(gmsd=0.062914, ms_gmsd=0.069569, haarpsi=0.656057, msdi=0.305328, vif_p=0.715699),
            2: dict(gmsd=0.060136, ms_gmsd=0.066521, haarpsi=0.711206, msdi=0.362868, vif_p=0.742840)}
    for i, w in want.items():
        p, t = pairs[i]
        got = E.all_metrics(p[:1], t[:1])
        for k, v in w.items():
            assert abs(got[k].item() - v) < 1.5e-6, (i, k, got[k].item(), v)


# ---- the collection's host side --------------------------------------------------------------------------------------
def _norms():
    from xmm_superres_denoise.transforms import Normalize
    return Normalize(1.0, 1.0, "sqrt"), [Normalize(1.0, 1.0, "linear"), Normalize(1.0, 1.0, "asinh")]


def test_key_names_and_signatures():
    from xmm_superres_denoise import metrics as M
    from xmm_superres_denoise import train
    dn, sc = _norms()
    for fn in (M.get_ext_metrics, M.get_in_ext_metrics):
        assert list(inspect.signature(fn).parameters) == ["dataset_normalizer", "scaling_normalizers", "prefix"]
    c = M.get_ext_metrics(dn, sc, "test")
    assert c.names == ("vif_p", "gmsd", "ms_gmsd", "haarpsi", "msdi") and set(c.states) == {"linear", "asinh"}
    ci = M.get_in_ext_metrics(dataset_normalizer=dn, scaling_normalizers=sc, prefix="test")
    vals = torch.tensor([[0.1, 0.2, 0.3, 0.4, 1.0, 2.0]], dtype=F64)
    for coll in (c, ci):
        for st in coll.states.values():
            st.add(vals)
    assert set(c.compute()) == {f"test/{m}/{n}" for m in ("linear", "asinh") for n in M.EXT_NAMES}
    assert set(ci.compute()) == {f"test/{m}/in/{n}" for m in ("linear", "asinh") for n in M.EXT_NAMES}
    assert abs(c.compute()["test/linear/vif_p"].item() - 0.5) < 1e-7 and abs(ci.compute()["test/asinh/in/msdi"].item() - 0.4) < 1e-7
    for fn in (train.fit, train.test):
        assert inspect.signature(fn).parameters["extended_metrics"].default is False
    assert "fsim" in train.EXT_METRICS_ON_NOTICE and "parity unpinned" in train.EXT_METRICS_ON_NOTICE
    assert "not computed" in train.EXT_METRICS_NOTICE


def test_epoch_reduction_is_the_references():
    """piq wrappers (metrics/metrics.py:9-27): sum of per-batch MEANS / number of images; vif_p: sum of per-image values / number of
    images.  Hand-made per-image values, batches of 2 and 3 images."""
    from xmm_superres_denoise.metrics import ExtEpochState
    b1 = torch.tensor([[0.10, 0.20, 0.90, 0.30, 6.0, 8.0], [0.30, 0.40, 0.70, 0.50, 1.0, 4.0]], dtype=F64)
    b2 = torch.tensor([[0.20, 0.10, 0.60, 0.10, 3.0, 4.0], [0.50, 0.30, 0.30, 0.20, 2.0, 8.0], [0.80, 0.20, 0.90, 0.60, 5.0, 5.0]], dtype=F64)
    st = ExtEpochState()
    st.add(b1)
    st.add(b2)
    got = {k: v.item() for k, v in st.compute().items()}
    assert abs(got["gmsd"] - (0.2 + 0.5) / 5) < 1e-15                 # (mean of batch 1 + mean of batch 2) / 5, NOT the mean of the five (0.38)
    assert abs(got["ms_gmsd"] - (0.3 + 0.2) / 5) < 1e-15
    assert abs(got["haarpsi"] - (0.8 + 0.6) / 5) < 1e-15
    assert abs(got["msdi"] - (0.4 + 0.3) / 5) < 1e-15
    assert abs(got["vif_p"] - (0.75 + 0.25 + 0.75 + 0.25 + 1.0) / 5) < 1e-15
    want = E.reduce_epoch([{"gmsd": b[:, 0], "ms_gmsd": b[:, 1], "haarpsi": b[:, 2], "msdi": b[:, 3], "vif_p": b[:, 4] / b[:, 5]} for b in (b1, b2)])
    assert all(abs(got[k] - want[k]) < 1e-15 for k in want)
    st.sync()             # no process group: a no-op
    assert abs(st.compute()["gmsd"].item() - 0.14) < 1e-15


def test_refusals_by_name():
    from xmm_superres_denoise.metrics import XMMExtMetricCollection, get_ext_metrics
    dn, sc = _norms()
    with pytest.raises(NotImplementedError, match="fsim"):
        XMMExtMetricCollection(("vif_p", "fsim"), dn, sc, "test")
    with pytest.raises(NotImplementedError, match="in/fsim"):
        XMMExtMetricCollection(("in/fsim",), dn, sc, "test")
    with pytest.raises(NotImplementedError, match="brisque"):
        XMMExtMetricCollection(("brisque",), dn, sc, "test")
    c = get_ext_metrics(dn, sc, "test")
    with pytest.raises(NotImplementedError, match="single-channel"):
        c.update(torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 64))
    with pytest.raises(NotImplementedError, match="single-channel"):
        c.update(torch.zeros(2, 64, 64), torch.zeros(2, 64, 64))
