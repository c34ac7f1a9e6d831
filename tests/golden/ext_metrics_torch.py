"""Plain-torch restatement of the extended test metrics (the reference's get_ext_metrics, metrics/metrics.py:42-101 with
every default and chromatic=False): gmsd, ms_gmsd, haarpsi, msdi (piq 0.7.x `mdsi`) and vif_p (torchmetrics 1.x
VisualInformationFidelity(sigma_n_sq=2.0)), for single-channel images in [0, 1].

piq and torchmetrics are not available to this project, so these formulas restate their published code and ARE the
project's specification: parity with the libraries themselves is unpinned, exactly as for
psnr / ssim / ms_ssim.  Everything is dtype-generic: float64 is the yardstick of tests/test_hip_ext_metrics.py, float32 is
"what the reference's arithmetic gives".  Inputs: x = preds, y = target, [B, H, W] (or [B, 1, H, W]); every function
returns per-image values [B].  fsim is not restated (it is refused by the engine: it needs 2-D FFTs of sizes the engine's
FFT does not take, plus a per-image median).
"""
import math

import torch
import torch.nn.functional as F

NAMES = ("vif_p", "gmsd", "ms_gmsd", "haarpsi", "msdi")
MS_GMSD_WEIGHTS = (0.096, 0.596, 0.289, 0.019)
EPS32 = float(torch.finfo(torch.float32).eps)


def _b1hw(x):
    return x[:, None] if x.dim() == 3 else x


def prewitt_grad(x):
    """sqrt(Px^2 + P^T x^2) with P = [[-1, 0, 1]] * 3 / 3 as a zero-padded (pad 1) correlation; x [B,1,H,W]"""
    k = torch.tensor([[-1.0, 0.0, 1.0]] * 3, dtype=x.dtype, device=x.device) / 3
    g = F.conv2d(x, torch.stack([k, k.t()])[:, None], padding=1)
    return torch.sqrt((g ** 2).sum(1, keepdim=True))


def sim(a, b, c):
    return (2 * a * b + c) / (a ** 2 + b ** 2 + c)


def pool2(x):
    """zero-pad by d = max(H % 2, W % 2) on the right AND the bottom, then 2x2 average, stride 2"""
    d = max(x.shape[-2] % 2, x.shape[-1] % 2)
    return F.avg_pool2d(F.pad(x, [0, d, 0, d]), 2, 2, 0)


def _pstd(g):
    m = g.mean(dim=[1, 2, 3], keepdim=True)
    return ((g - m) ** 2).mean(dim=[1, 2, 3]).sqrt()


def gmsd(x, y):
    x, y = pool2(_b1hw(x)), pool2(_b1hw(y))
    t = 170 / 255 ** 2
    a, b = prewitt_grad(x), prewitt_grad(y)
    return _pstd((2 * a * b + t) / (a ** 2 + b ** 2 + t))


def ms_gmsd_scales(x, y, alpha=0.5, t=170.0):
    """the four per-scale deviations s_k, [B, 4]"""
    x, y = 255 * _b1hw(x), 255 * _b1hw(y)
    out = []
    for k in range(4):
        if k > 0:
            x, y = pool2(x), pool2(y)
        a, b = prewitt_grad(x), prewitt_grad(y)
        out.append(_pstd(((2 - alpha) * a * b + t) / (a ** 2 + b ** 2 - alpha * a * b + t)))
    return torch.stack(out, 1)


def ms_gmsd(x, y):
    s = ms_gmsd_scales(x, y)
    w = torch.tensor(MS_GMSD_WEIGHTS, dtype=s.dtype, device=s.device)
    return torch.sqrt((w[None] * s ** 2).sum(1))


def haar_coefficients(x, scale):
    """[B, 2, H, W]: correlation with the k x k Haar kernel (k = 2^(scale+1)) and its transpose, zero-padded by k/2 - 1
    (left / top) and k/2 (right / bottom)"""
    k = 2 ** (scale + 1)
    h = torch.ones(k, k, dtype=x.dtype, device=x.device) / k
    h[k // 2:, :] = -h[k // 2:, :]
    up, lo = k // 2 - 1, k // 2
    return F.conv2d(F.pad(x, [up, lo, up, lo]), torch.stack([h, h.t()])[:, None])


def haarpsi_parts(x, y, c=30.0, alpha=4.2):
    """(sum_o sum_px sigmoid(alpha S_o) w_o, sum_o sum_px w_o), each [B]"""
    x, y = pool2(255 * _b1hw(x)), pool2(255 * _b1hw(y))
    cx = [haar_coefficients(x, s).abs() for s in range(3)]
    cy = [haar_coefficients(y, s).abs() for s in range(3)]
    w = torch.maximum(cx[2], cy[2])
    s = (sim(cx[0], cy[0], c) + sim(cx[1], cy[1], c)) / 2
    return (torch.sigmoid(alpha * s) * w).sum(dim=[1, 2, 3]), w.sum(dim=[1, 2, 3])


def haarpsi(x, y, alpha=4.2):
    n, d = haarpsi_parts(x, y, alpha=alpha)
    v = (n + EPS32) / (d + EPS32)
    return (torch.log(v / (1 - v)) / alpha) ** 2


def mdsi_kernel_size(H, W):
    return max(1, round(min(H, W) / 256))


def mdsi_pool(x):
    k = mdsi_kernel_size(*x.shape[-2:])
    if k > 1:
        x = F.pad(x, [(k - 1) // 2, k // 2, (k - 1) // 2, k // 2])
    return F.avg_pool2d(x, k)


def complex_power(g, q):
    """(re, im) of g^q for real g as piq takes it: |g|^q at the argument q * atan2(0, g), i.e. q * pi where g < 0"""
    mag = g.abs() ** q
    ang = torch.where(g < 0, torch.full_like(g, q * math.pi), torch.zeros_like(g))
    return mag * torch.cos(ang), mag * torch.sin(ang)


def mdsi_deviation(x, y, c1=140.0, c2=55.0, c3=550.0, alpha=0.6, q=0.25, rho=1.0):
    """mean_px |z - mean_px z|^rho with z = G^q as a complex power: what the o / rho root is taken of, [B]"""
    x, y = mdsi_pool(_b1hw(x)), mdsi_pool(_b1hw(y))
    lx, hx, mx = 0.9999 * (255 * x), -0.01 * (255 * x), -0.09 * (255 * x)
    ly, hy, my = 0.9999 * (255 * y), -0.01 * (255 * y), -0.09 * (255 * y)
    gx, gy, ga = prewitt_grad(lx), prewitt_grad(ly), prewitt_grad((lx + ly) / 2)
    gs = sim(gx, gy, c1) + sim(gx, ga, c2) - sim(gy, ga, c2)
    cs = (2 * (hx * hy + mx * my) + c3) / (hx ** 2 + hy ** 2 + mx ** 2 + my ** 2 + c3)
    g = alpha * gs + (1 - alpha) * cs
    re, im = complex_power(g, q)
    mre, mim = re.mean(dim=[1, 2, 3], keepdim=True), im.mean(dim=[1, 2, 3], keepdim=True)
    dev = torch.sqrt((re - mre) ** 2 + (im - mim) ** 2)
    return (dev ** rho).mean(dim=[1, 2, 3])


def msdi(x, y, o=0.25, rho=1.0):
    return mdsi_deviation(x, y, rho=rho) ** (o / rho)


def vif_kernel(n, dtype, device=None):
    c = torch.arange(-(n // 2), n // 2 + 1, dtype=dtype, device=device)
    g = torch.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2.0 * (n / 3) ** 2))
    return (g / g.sum())[None, None]


def vif_parts(x, y, sigma_n_sq=2.0):
    """(numerator, denominator), each [B]; x = preds, y = target"""
    p, t = _b1hw(x), _b1hw(y)
    eps = 1e-10
    num = torch.zeros(p.shape[0], dtype=p.dtype, device=p.device)
    den = torch.zeros_like(num)
    for s in range(4):
        n = 2 ** (4 - s) + 1
        k = vif_kernel(n, p.dtype, p.device)
        if s > 0:
            t, p = F.conv2d(t, k)[:, :, ::2, ::2], F.conv2d(p, k)[:, :, ::2, ::2]
        mu_t, mu_p = F.conv2d(t, k), F.conv2d(p, k)
        st = torch.clamp(F.conv2d(t ** 2, k) - mu_t ** 2, min=0.0)
        sp = torch.clamp(F.conv2d(p ** 2, k) - mu_p ** 2, min=0.0)
        stp = F.conv2d(t * p, k) - mu_t * mu_p
        g = stp / (st + eps)
        sv = sp - g * stp
        m = st < eps
        g = torch.where(m, torch.zeros_like(g), g)
        sv = torch.where(m, sp, sv)
        st = torch.where(m, torch.zeros_like(st), st)
        m = sp < eps
        g = torch.where(m, torch.zeros_like(g), g)
        sv = torch.where(m, torch.zeros_like(sv), sv)
        m = g < 0
        sv = torch.where(m, sp, sv)
        g = torch.where(m, torch.zeros_like(g), g)
        sv = torch.clamp(sv, min=eps)
        num = num + torch.log10(1.0 + g ** 2 * st / (sv + sigma_n_sq)).sum(dim=[1, 2, 3])
        den = den + torch.log10(1.0 + st / sigma_n_sq).sum(dim=[1, 2, 3])
    return num, den


def vif_p(x, y):
    n, d = vif_parts(x, y)
    return n / d


# ---- the same formulas returning MAPS, not sums: the per-stage yardstick of tests/test_hip_ext_metrics_kernels.py.  Every map is
# [B, h, w] in the dtype of the inputs; reduced, they are the functions above (tests/test_hip_ext_metrics_kernels.py asserts it).
def pool_levels(x):
    """[pool2(x), pool2^2(x), pool2^3(x)] of a [B, H, W] image, each [B, h, w]"""
    out, u = [], _b1hw(x)
    for _ in range(3):
        u = pool2(u)
        out.append(u[:, 0])
    return out


def gms_maps(x, y, alpha=0.5, t=170.0):
    """([MS-GMSD's similarity map at scales 0..3], GMSD's similarity map (on the once-pooled [0, 1] image))"""
    a, b = 255 * _b1hw(x), 255 * _b1hw(y)
    ms = []
    for k in range(4):
        if k > 0:
            a, b = pool2(a), pool2(b)
        ga, gb = prewitt_grad(a), prewitt_grad(b)
        ms.append((((2 - alpha) * ga * gb + t) / (ga ** 2 + gb ** 2 - alpha * ga * gb + t))[:, 0])
    a, b = pool2(_b1hw(x)), pool2(_b1hw(y))
    t1 = 170 / 255 ** 2
    ga, gb = prewitt_grad(a), prewitt_grad(b)
    return ms, ((2 * ga * gb + t1) / (ga ** 2 + gb ** 2 + t1))[:, 0]


def haarpsi_maps(x, y, c=30.0, alpha=4.2):
    """(sum_o sigmoid(alpha S_o) w_o, sum_o w_o) per pixel of the once-pooled image"""
    x, y = pool2(255 * _b1hw(x)), pool2(255 * _b1hw(y))
    cx = [haar_coefficients(x, s).abs() for s in range(3)]
    cy = [haar_coefficients(y, s).abs() for s in range(3)]
    w = torch.maximum(cx[2], cy[2])
    s = (sim(cx[0], cy[0], c) + sim(cx[1], cy[1], c)) / 2
    return (torch.sigmoid(alpha * s) * w).sum(1), w.sum(1)


def mdsi_maps(x, y, c1=140.0, c2=55.0, c3=550.0, alpha=0.6, q=0.25):
    """(pooled x, pooled y, re z, im z, |z - mean z|) with z = G^q as a complex power"""
    x, y = mdsi_pool(_b1hw(x)), mdsi_pool(_b1hw(y))
    lx, hx, mx = 0.9999 * (255 * x), -0.01 * (255 * x), -0.09 * (255 * x)
    ly, hy, my = 0.9999 * (255 * y), -0.01 * (255 * y), -0.09 * (255 * y)
    gx, gy, ga = prewitt_grad(lx), prewitt_grad(ly), prewitt_grad((lx + ly) / 2)
    gs = sim(gx, gy, c1) + sim(gx, ga, c2) - sim(gy, ga, c2)
    cs = (2 * (hx * hy + mx * my) + c3) / (hx ** 2 + hy ** 2 + mx ** 2 + my ** 2 + c3)
    re, im = complex_power(alpha * gs + (1 - alpha) * cs, q)
    mre, mim = re.mean(dim=[1, 2, 3], keepdim=True), im.mean(dim=[1, 2, 3], keepdim=True)
    return x[:, 0], y[:, 0], re[:, 0], im[:, 0], torch.sqrt((re - mre) ** 2 + (im - mim) ** 2)[:, 0]


def vif_maps(x, y, sigma_n_sq=2.0):
    """per scale 0..3: (preds image, target image, numerator map, denominator map); the maps are over the valid windows"""
    p, t = _b1hw(x), _b1hw(y)
    eps = 1e-10
    out = []
    for s in range(4):
        n = 2 ** (4 - s) + 1
        k = vif_kernel(n, p.dtype, p.device)
        if s > 0:
            t, p = F.conv2d(t, k)[:, :, ::2, ::2], F.conv2d(p, k)[:, :, ::2, ::2]
        mu_t, mu_p = F.conv2d(t, k), F.conv2d(p, k)
        st = torch.clamp(F.conv2d(t ** 2, k) - mu_t ** 2, min=0.0)
        sp = torch.clamp(F.conv2d(p ** 2, k) - mu_p ** 2, min=0.0)
        stp = F.conv2d(t * p, k) - mu_t * mu_p
        g = stp / (st + eps)
        sv = sp - g * stp
        m = st < eps
        g = torch.where(m, torch.zeros_like(g), g)
        sv = torch.where(m, sp, sv)
        st = torch.where(m, torch.zeros_like(st), st)
        m = sp < eps
        g = torch.where(m, torch.zeros_like(g), g)
        sv = torch.where(m, torch.zeros_like(sv), sv)
        m = g < 0
        sv = torch.where(m, sp, sv)
        g = torch.where(m, torch.zeros_like(g), g)
        sv = torch.clamp(sv, min=eps)
        out.append((p[:, 0], t[:, 0], torch.log10(1.0 + g ** 2 * st / (sv + sigma_n_sq))[:, 0], torch.log10(1.0 + st / sigma_n_sq)[:, 0]))
    return out


def tile_sums(m, th, tw):
    """[B, h, w] -> [B, ntiles]: the sum over each th x tw tile, tiles in row-major order (the last row / column of tiles may be partial)"""
    B, h, w = m.shape
    ny, nx = -(-h // th), -(-w // tw)
    m = F.pad(m, [0, nx * tw - w, 0, ny * th - h])
    return m.reshape(B, ny, th, nx, tw).sum(dim=[2, 4]).reshape(B, ny * nx)


FUNCS = {"vif_p": vif_p, "gmsd": gmsd, "ms_gmsd": ms_gmsd, "haarpsi": haarpsi, "msdi": msdi}


def all_metrics(x, y):
    """{name: [B] tensor} for the five metrics"""
    return {n: FUNCS[n](x, y) for n in NAMES}


def photon_pair(shape, gen, dtype=torch.float64, rate=0.3, noise=0.05):
    """photon-like test pair: target = 3x3-smoothed clamped Poisson counts, prediction = target + noise clamped to [0, 1]"""
    t = torch.poisson(torch.full(shape, rate, dtype=dtype), generator=gen)
    t = F.avg_pool2d(torch.clamp(t / 6, 0, 1)[:, None], 3, 1, 1)[:, 0]
    p = torch.clamp(t + noise * torch.randn(shape, dtype=dtype, generator=gen), 0, 1)
    return p, t


def reduce_epoch(per_batch):
    """The reference's epoch reduction (metrics/metrics.py:9-27) of a list of per-batch {name: [B] per-image values}: the five
    piq wrappers add the BATCH MEAN to `metric` and B to `total` and report metric / total; vif_p is torchmetrics' own class,
    sum of per-image values / number of images."""
    out = {}
    for n in NAMES:
        tot = sum(int(b[n].numel()) for b in per_batch)
        if n == "vif_p":
            out[n] = sum(float(b[n].double().sum()) for b in per_batch) / tot
        else:
            out[n] = sum(float(b[n].double().mean()) for b in per_batch) / tot
    return out
