"""Plain-torch restatement of `piq.fsim(x, y, chromatic=False)` with the defaults of piq 0.7.x (data_range=1.0, scales=4,
orientations=4, min_length=6, mult=2, sigma_f=0.55, delta_theta=1.2, k=2.0), per image (reduction="none"): the sixth of the
reference's extended test metrics (metrics/xmm_metric_collection.py:41-61), for single-channel images in [0, 1].

piq is not available to this project, so this file restates its published code and IS the project's specification of the
metric: PARITY WITH piq ITSELF IS UNPINNED, exactly as for the five metrics of
ext_metrics_torch.py.  Everything is dtype-generic: float64 is the yardstick of tests/test_hip_fsim.py, float32 is "what the
reference's arithmetic gives".  Inputs: x = preds, y = target, [B, H, W] (or [B, 1, H, W]); `fsim` returns per-image values [B].

One known difference from piq's published code, stated in DESIGN.md section 17: the phase congruency is sum(energy) / sum(an) with no
epsilon added to either sum, so a pair without any structure (sum(pc_max) = 0: two all-zero images) gives NaN, where piq's epsilons
give 1.  As in piq, pc_max is where(pc_x > pc_y, pc_x, pc_y) and the median is taken of (sqrt(e^2 + o^2))^2.
"""
import math

import torch
import torch.nn.functional as F

SCALES, ORIENTATIONS, MIN_LENGTH, MULT, SIGMA_F, DELTA_THETA, K = 4, 4, 6, 2, 0.55, 1.2, 2.0
T1, T2 = 0.85, 160.0


def _b1hw(x):
    return x[:, None] if x.dim() == 3 else x


def kernel_size(H, W):
    """Python's round: ties to even (640 -> 2, 384 -> 2)"""
    return max(1, round(min(H, W) / 256))


def pool(x):
    """255 * x, then the ks x ks mean without padding (the remainder rows / columns are dropped); x [B,1,H,W]"""
    return F.avg_pool2d(x * 255, kernel_size(*x.shape[-2:]))


def pooled_size(H, W):
    ks = kernel_size(H, W)
    return H // ks, W // ks


def _axis(n, dtype):
    if n % 2:
        return torch.arange(-(n - 1) / 2, n / 2, dtype=dtype) / (n - 1)
    return torch.arange(-n / 2, n / 2, dtype=dtype) / n


def _ifftshift(x):
    return torch.roll(x, [-(n // 2) for n in x.shape], list(range(x.dim())))


def grid(h, w, dtype):
    """(radius, theta) on the unshifted frequency grid; the first axis (rows) is piq's grid_x"""
    gx, gy = torch.meshgrid(_axis(h, dtype), _axis(w, dtype), indexing="ij")
    return _ifftshift(torch.sqrt(gx ** 2 + gy ** 2)), _ifftshift(torch.atan2(-gy, gx))


def lowpass(h, w, dtype, cutoff=0.45, n=15):
    radius, _ = grid(h, w, dtype)
    return 1.0 / (1.0 + (radius / cutoff) ** (2 * n))


def construct_filters(h, w, dtype):
    """[ORIENTATIONS, SCALES, h, w] real log-Gabor filters (piq's _construct_filters)"""
    radius, theta = grid(h, w, dtype)
    radius[0, 0] = 1
    sintheta, costheta = torch.sin(theta), torch.cos(theta)
    lp = lowpass(h, w, dtype)
    theta_sigma = math.pi / (ORIENTATIONS * DELTA_THETA)
    log_gabor = []
    for s in range(SCALES):
        omega_0 = 1.0 / (MIN_LENGTH * MULT ** s)
        g = torch.exp(-(torch.log(radius / omega_0) ** 2) / (2 * math.log(SIGMA_F) ** 2)) * lp
        g[0, 0] = 0
        log_gabor.append(g)
    spread = []
    for o in range(ORIENTATIONS):
        angl = o * math.pi / ORIENTATIONS
        ds = sintheta * math.cos(angl) - costheta * math.sin(angl)
        dc = costheta * math.cos(angl) + sintheta * math.sin(angl)
        dtheta = torch.abs(torch.atan2(ds, dc))
        spread.append(torch.exp(-(dtheta ** 2) / (2 * theta_sigma ** 2)))
    return torch.stack(spread)[:, None] * torch.stack(log_gabor)[None]


def noise_constants(filters):
    """per orientation: em_n, sum_an2, sum_ai_aj (each [ORIENTATIONS]); they depend on (h, w) only"""
    h, w = filters.shape[-2:]
    em_n = (filters[:, 0] ** 2).sum(dim=[-2, -1])
    g = torch.fft.ifft2(filters).real * math.sqrt(h * w)
    sum_an2 = (g ** 2).sum(dim=[1, 2, 3])
    sum_ai_aj = torch.zeros_like(sum_an2)
    for s in range(SCALES - 1):
        sum_ai_aj = sum_ai_aj + (g[:, s:s + 1] * g[:, s + 1:]).sum(dim=[1, 2, 3])
    return em_n, sum_an2, sum_ai_aj


def phase_congruency(img, parts=False):
    """img [B,1,h,w] (pooled, 255-scaled) -> pc [B,1,h,w] (piq's _phase_congruency)"""
    eps = torch.finfo(img.dtype).eps
    B, _, h, w = img.shape
    filters = construct_filters(h, w, img.dtype).to(img.device)
    em_n, sum_an2, sum_ai_aj = (c.reshape(1, ORIENTATIONS, 1, 1) for c in noise_constants(filters))
    eo = torch.fft.ifft2(torch.fft.fft2(img)[:, :, None] * filters[None])          # [B, O, S, h, w] complex
    even, odd = eo.real, eo.imag
    an = torch.sqrt(even ** 2 + odd ** 2)
    sum_e, sum_o = even.sum(2, keepdim=True), odd.sum(2, keepdim=True)
    x_energy = torch.sqrt(sum_e ** 2 + sum_o ** 2) + eps
    mean_e, mean_o = sum_e / x_energy, sum_o / x_energy
    energy = (even * mean_e + odd * mean_o - torch.abs(even * mean_o - odd * mean_e)).sum(2)       # [B, O, h, w]
    median_e2n = torch.median((an[:, :, 0] ** 2).reshape(B, ORIENTATIONS, h * w), dim=-1).values.reshape(B, ORIENTATIONS, 1, 1)
    mean_e2n = -median_e2n / math.log(0.5)
    noise_power = mean_e2n / em_n
    noise_energy2 = 2 * noise_power * sum_an2 + 4 * noise_power * sum_ai_aj
    tau = torch.sqrt(noise_energy2 / 2)
    T = (tau * math.sqrt(math.pi / 2) + K * torch.sqrt((2 - math.pi / 2) * tau ** 2)) / 1.7
    energy = torch.max(energy - T, torch.zeros_like(energy))
    pc = (energy.sum(1) / an.sum(dim=[1, 2]))[:, None]
    if parts:
        return pc, {"eo": eo, "T": T.reshape(B, ORIENTATIONS), "median": median_e2n.reshape(B, ORIENTATIONS)}
    return pc


def scharr_grad(x):
    """sqrt(gx^2 + gy^2), Scharr kernel / 16 and its transpose as a zero-padded (pad 1) correlation; x [B,1,h,w]"""
    k = torch.tensor([[-3.0, 0.0, 3.0], [-10.0, 0.0, 10.0], [-3.0, 0.0, 3.0]], dtype=x.dtype, device=x.device) / 16
    g = F.conv2d(x, torch.stack([k, k.t()])[:, None], padding=1)
    return torch.sqrt((g ** 2).sum(1, keepdim=True))


def sim(a, b, c):
    return (2 * a * b + c) / (a ** 2 + b ** 2 + c)


def fsim_parts(x, y):
    """(sum(GM * PC * pc_max), sum(pc_max)), each [B]"""
    x, y = pool(_b1hw(x)), pool(_b1hw(y))
    pc_x, pc_y = phase_congruency(x), phase_congruency(y)
    g_x, g_y = scharr_grad(x), scharr_grad(y)
    pc_max = torch.where(pc_x > pc_y, pc_x, pc_y)
    score = sim(g_x, g_y, T2) * sim(pc_x, pc_y, T1) * pc_max
    return score.sum(dim=[1, 2, 3]), pc_max.sum(dim=[1, 2, 3])


def fsim(x, y):
    n, d = fsim_parts(x, y)
    return n / d


# ---- the same formulas returning every intermediate MAP: the per-stage yardstick of tests/test_hip_fsim_kernels.py (reduced, they are
# the functions above; that file asserts it)
def pc_maps(img):
    """img [B,1,h,w] (pooled, 255-scaled) -> dict: eo [B,O,S,h,w] complex; en [B,O,h,w] the energy BEFORE its threshold; an [B,O,h,w] the
    sum over the scales of |eo|; a0sq [B,O,h,w] = |eo[:, :, 0]|^2 (what the median is taken of); T [B,O]; pc [B,h,w]"""
    eps = torch.finfo(img.dtype).eps
    B, _, h, w = img.shape
    filters = construct_filters(h, w, img.dtype).to(img.device)
    em_n, sum_an2, sum_ai_aj = (c.reshape(1, ORIENTATIONS, 1, 1) for c in noise_constants(filters))
    eo = torch.fft.ifft2(torch.fft.fft2(img)[:, :, None] * filters[None])
    even, odd = eo.real, eo.imag
    an = torch.sqrt(even ** 2 + odd ** 2)
    sum_e, sum_o = even.sum(2, keepdim=True), odd.sum(2, keepdim=True)
    x_energy = torch.sqrt(sum_e ** 2 + sum_o ** 2) + eps
    mean_e, mean_o = sum_e / x_energy, sum_o / x_energy
    en = (even * mean_e + odd * mean_o - torch.abs(even * mean_o - odd * mean_e)).sum(2)
    a0sq = an[:, :, 0] ** 2
    T = threshold(torch.median(a0sq.reshape(B, ORIENTATIONS, h * w), dim=-1).values.reshape(B, ORIENTATIONS, 1, 1), em_n, sum_an2, sum_ai_aj)
    pc = torch.max(en - T, torch.zeros_like(en)).sum(1) / an.sum(dim=[1, 2])
    return {"eo": eo, "en": en, "an": an.sum(2), "a0sq": a0sq, "T": T.reshape(B, ORIENTATIONS), "pc": pc}


def threshold(median_e2n, em_n, sum_an2, sum_ai_aj):
    """the noise threshold T of an orientation from the median of |eo[o, 0]|^2 and the orientation's three noise constants"""
    mean_e2n = -median_e2n / math.log(0.5)
    noise_power = mean_e2n / em_n
    noise_energy2 = 2 * noise_power * sum_an2 + 4 * noise_power * sum_ai_aj
    tau = torch.sqrt(noise_energy2 / 2)
    return (tau * math.sqrt(math.pi / 2) + K * torch.sqrt((2 - math.pi / 2) * tau ** 2)) / 1.7


def fsim_maps(x, y):
    """dict: pooled [2][B,h,w] (preds, target); pc [2] of pc_maps' dicts; num = GM * PC * pc_max and den = pc_max, each [B,h,w]"""
    x, y = pool(_b1hw(x)), pool(_b1hw(y))
    mx, my = pc_maps(x), pc_maps(y)
    pc_x, pc_y = mx["pc"][:, None], my["pc"][:, None]
    g_x, g_y = scharr_grad(x), scharr_grad(y)
    pc_max = torch.where(pc_x > pc_y, pc_x, pc_y)
    score = sim(g_x, g_y, T2) * sim(pc_x, pc_y, T1) * pc_max
    return {"pooled": (x[:, 0], y[:, 0]), "pc": (mx, my), "num": score[:, 0], "den": pc_max[:, 0]}


def photon_pair(shape, gen, dtype=torch.float64, rate=0.3, noise=0.05):
    """photon-like test pair, made as tests/test_hip_ext_metrics.py makes its pairs: target = 3x3-smoothed clamped Poisson counts,
    prediction = target + noise clamped to [0, 1]"""
    t = torch.poisson(torch.full(shape, rate, dtype=dtype), generator=gen)
    t = F.avg_pool2d(torch.clamp(t / 6, 0, 1)[:, None], 3, 1, 1)[:, 0]
    p = torch.clamp(t + noise * torch.randn(shape, dtype=dtype, generator=gen), 0, 1)
    return p, t


# the cases of tests/golden/fsim_cases.npz and of the GPU accuracy test: name -> (H, W, images); seed = 100 + H + W as in
# test_hip_ext_metrics.py
CASES = {"61x53": (61, 53, 4), "64x48": (64, 48, 4), "417x403": (417, 403, 4), "832x832": (832, 832, 1)}


def case_pair(name):
    """the seeded pair of a case, rounded to fp32 (what the engine sees)"""
    H, W, B = CASES[name]
    p, t = photon_pair((B, H, W), torch.Generator().manual_seed(100 + H + W))
    return p.float(), t.float()


def reduce_epoch(per_batch):
    """The reference's `_Metric` epoch reduction (metrics/metrics.py:9-27,92-101) of a list of per-batch [B] per-image values: the
    BATCH MEAN is added to `metric`, B to `total`; the value is metric / total."""
    return sum(float(b.double().mean()) for b in per_batch) / sum(int(b.numel()) for b in per_batch)
