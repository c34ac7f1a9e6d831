// ext_metrics.hip -- the reference's extended test metrics (metrics/xmm_metric_collection.py:41-61: get_ext_metrics) on
// single-channel [0, 1] images: gmsd, ms_gmsd, haarpsi, mdsi (piq 0.7.x, chromatic=False) and the pixel-domain VIF of
// torchmetrics 1.x (sigma_n_sq = 2).  The formulas are restated from the libraries' published code (include/xsd.h;
// DESIGN.md section 14): parity with the libraries themselves is unpinned, as for psnr / ssim / ms_ssim.
//
// One xsd_ext_metrics_eval is a fixed chain of 11 launches, whatever B is (blockIdx.y = image):
//    1  pool_chain      x, y -> the three pool2 levels U1..U3 (one thread owns a 4x4 / 2x2 / 1 cell of the three levels)
//    2  mdsi_pool       x, y -> the k x k averaged images MDSI works on
//  3-5  vif_decimate    the 9 / 5 / 3 tap valid Gaussian + [::2, ::2] chain V1..V3 of VIF's scales 1..3
//    6  gms             blockIdx.z = scale 0..3: Prewitt gradients -> MS-GMSD's similarity map (and GMSD's at scale 1) -> sums
//    7  haarpsi         the three Haar scales from one 8x8 neighbourhood (LDS tile with halo) -> weighted sigmoid sums
//    8  mdsi_pass1      complex G^q map -> sums of its real / imaginary part
//    9  mdsi_pass2      the same map again, now against its mean -> sum of |z - mean z|
//   10  vif_stats       blockIdx.z = scale 0..3: windowed moments (LDS pixel tile, separable Gaussian) -> the two log10 sums
//   11  finish          one workgroup per image: tile partials -> the six values
// The maps are fp32; everything summed over an image is a double.  Every workgroup reduces its tile (64 x 4 pixels; 16 x 16 windows
// in vif_stats) in a fixed
// order (wave shuffles, then the four waves) into its own slot of a partial array; `finish` adds an image's slots in a
// fixed order.  No atomics: an image's values do not depend on its batch-mates or on the run, and a NaN stays in its image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>

#include "../../include/xsd.h"

#include "xsd_err.h"
#include "xsd_mem.h"
#define fail xsd::failf      // the thread-local message of xsd_last_error()

namespace {

constexpr int TW = 64, TH = 4, NT = TW * TH;      // one workgroup = a 64 x 4 tile of a map = four waves, one per row
constexpr int NSCALE = 4;
constexpr int VIF_TAPS[NSCALE] = {17, 9, 5, 3};   // n = 2^(4-s) + 1

struct Plane {            // one image level: B images of h x w, x (preds) and y (target)
    const float* x;
    const float* y;
    int h, w;
};

struct ScaleSet {         // the four levels a multi-scale kernel walks with blockIdx.z, and where each puts its partials
    Plane p[NSCALE];
    double* part[NSCALE];
    int tiles_x[NSCALE], ntiles[NSCALE];
};

struct VifWeights {       // normalised 1-D Gaussians, sigma = n / 3; the 2-D window is their outer product
    float g[NSCALE][17];
};

struct PoolDims {
    int H, W, h1, w1, h2, w2, h3, w3;
};

struct FinishArgs {
    const double* gms[NSCALE];      // 4 per tile: sum g, sum g^2 (MS-GMSD form), sum g, sum g^2 (GMSD form, scale 1 only)
    const double* vif[NSCALE];      // 2 per tile: numerator, denominator
    int gms_tiles[NSCALE], vif_tiles[NSCALE];
    double gms_count[NSCALE];
    const double* haar;             // 2 per tile
    const double* mdsi2;            // 1 per tile
    int haar_tiles, mdsi_tiles;
    double mdsi_count;
};

__device__ __forceinline__ float ldz(const float* __restrict__ p, int h, int w, int i, int j)
{
    return (i >= 0 && i < h && j >= 0 && j < w) ? p[(size_t)i * w + j] : 0.f;
}

__device__ __forceinline__ void load3x3(const float* __restrict__ p, int h, int w, int i, int j, float (&n)[9])
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) n[a * 3 + b] = ldz(p, h, w, i + a - 1, j + b - 1);
}

// sqrt(Px^2 + P^T x^2), P = [[-1, 0, 1]] * 3 / 3, on a zero-padded 3 x 3 neighbourhood
__device__ __forceinline__ float grad9(const float (&n)[9])
{
    const float third = 1.f / 3.f;
    const float gx = ((n[2] - n[0]) + (n[5] - n[3]) + (n[8] - n[6])) * third;
    const float gy = ((n[6] - n[0]) + (n[7] - n[1]) + (n[8] - n[2])) * third;
    return sqrtf(gx * gx + gy * gy);
}

__device__ __forceinline__ float simf(float a, float b, float c) { return (2.f * a * b + c) / (a * a + b * b + c); }

// the workgroup's N sums, combined in a fixed order, into dst[0..N)
template <int N>
__device__ __forceinline__ void block_partials(const double (&v)[N], double* __restrict__ dst)
{
    __shared__ double sh[NT / 64][N];
    const int tid = threadIdx.y * TW + threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) sh[wv][k] = s;
    }
    __syncthreads();
    if (tid < N) dst[tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

// sum over an image's tiles of entry k of its N-wide partials, the same value in every thread: thread t adds tiles
// t, t + 256, ... in order, then the fixed workgroup tree
__device__ __forceinline__ double image_sum(const double* __restrict__ part, int ntiles, int N, int k)
{
    __shared__ double sh[NT / 64];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double s = 0.0;
    for (int t = tid; t < ntiles; t += NT) s += part[(size_t)t * N + k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __syncthreads();                      // the previous call's readers are done with sh
    if (lane == 0) sh[wv] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- 1: pool2 chain.  pool2 = zero-pad by d = max(h % 2, w % 2) right and bottom, 2x2 mean, stride 2 (floor); thread (ti, tj)
// owns U1[4ti..4ti+3][4tj..4tj+3], U2[2ti..2ti+1][2tj..2tj+1] and U3[ti][tj]; cells outside a level count as that level's zero pad
__global__ __launch_bounds__(NT) void pool_chain_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ ux,
                                                        float* __restrict__ uy, PoolDims d, int cells_x, int tiles_x)
{
    const int b = blockIdx.y;
    const float* src = (blockIdx.z ? y : x) + (size_t)b * d.H * d.W;
    float* u = blockIdx.z ? uy : ux;
    const size_t n1 = (size_t)d.h1 * d.w1, n2 = (size_t)d.h2 * d.w2, n3 = (size_t)d.h3 * d.w3;
    const size_t B = gridDim.y;
    float* u1 = u + (size_t)b * n1;
    float* u2 = u + B * n1 + (size_t)b * n2;
    float* u3 = u + B * (n1 + n2) + (size_t)b * n3;
    const int tj = (blockIdx.x % tiles_x) * TW + threadIdx.x, ti = (blockIdx.x / tiles_x) * TH + threadIdx.y;
    if (tj >= cells_x) return;
    float a1[4][4], a2[2][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = 4 * ti + r, j = 4 * tj + c;
            const bool in = i < d.h1 && j < d.w1;
            float v = 0.f;
            if (in) {
                v = 0.25f * ((ldz(src, d.H, d.W, 2 * i, 2 * j) + ldz(src, d.H, d.W, 2 * i, 2 * j + 1)) +
                             (ldz(src, d.H, d.W, 2 * i + 1, 2 * j) + ldz(src, d.H, d.W, 2 * i + 1, 2 * j + 1)));
                u1[(size_t)i * d.w1 + j] = v;
            }
            a1[r][c] = v;
        }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int i = 2 * ti + r, j = 2 * tj + c;
            const bool in = i < d.h2 && j < d.w2;
            const float v = in ? 0.25f * ((a1[2 * r][2 * c] + a1[2 * r][2 * c + 1]) + (a1[2 * r + 1][2 * c] + a1[2 * r + 1][2 * c + 1])) : 0.f;
            if (in) u2[(size_t)i * d.w2 + j] = v;
            a2[r][c] = v;
        }
    if (ti < d.h3 && tj < d.w3) u3[(size_t)ti * d.w3 + tj] = 0.25f * ((a2[0][0] + a2[0][1]) + (a2[1][0] + a2[1][1]));
}

// ---- 2: MDSI's pooling: zero-pad (k-1)/2 left / top, k/2 right / bottom, k x k mean with stride k
__global__ __launch_bounds__(NT) void mdsi_pool_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ mx,
                                                       float* __restrict__ my, int H, int W, int mh, int mw, int k, int tiles_x)
{
    const int b = blockIdx.y;
    const float* src = (blockIdx.z ? y : x) + (size_t)b * H * W;
    float* dst = (blockIdx.z ? my : mx) + (size_t)b * mh * mw;
    const int j = (blockIdx.x % tiles_x) * TW + threadIdx.x, i = (blockIdx.x / tiles_x) * TH + threadIdx.y;
    if (i >= mh || j >= mw) return;
    const int pl = (k - 1) / 2;
    float s = 0.f;
    for (int a = 0; a < k; ++a)
        for (int c = 0; c < k; ++c) s += ldz(src, H, W, i * k - pl + a, j * k - pl + c);
    dst[(size_t)i * mw + j] = s / (float)(k * k);
}

// ---- 3-5: one step of VIF's chain: valid N x N Gaussian, decimated [::2, ::2]; every tap is inside the h x w source
template <int N>
__device__ __forceinline__ float vif_window(const float* __restrict__ src, int w, int i0, int j0, const float* __restrict__ g)
{
    float s = 0.f;
#pragma unroll
    for (int dy = 0; dy < N; ++dy) {
        float r = 0.f;
#pragma unroll
        for (int dx = 0; dx < N; ++dx) r += g[dx] * src[(size_t)(i0 + dy) * w + j0 + dx];
        s += g[dy] * r;
    }
    return s;
}

// the scale's 1-D weights, from the kernel's argument block into LDS (every thread of the workgroup calls this)
__device__ __forceinline__ const float* vif_taps_to_lds(const VifWeights& vw, int scale)
{
    __shared__ float g[17];
    const int tid = threadIdx.y * TW + threadIdx.x;
    if (tid < 17) g[tid] = vw.g[scale][tid];
    __syncthreads();
    return g;
}

__global__ __launch_bounds__(NT) void vif_decimate_kernel(Plane in, float* __restrict__ ox, float* __restrict__ oy, int oh, int ow, int scale,
                                                          VifWeights vw, int tiles_x)
{
    const int b = blockIdx.y;
    const float* src = (blockIdx.z ? in.y : in.x) + (size_t)b * in.h * in.w;
    float* dst = (blockIdx.z ? oy : ox) + (size_t)b * oh * ow;
    const int j = (blockIdx.x % tiles_x) * TW + threadIdx.x, i = (blockIdx.x / tiles_x) * TH + threadIdx.y;
    const float* g = vif_taps_to_lds(vw, scale);
    if (i >= oh || j >= ow) return;
    float v;
    if (scale == 1) v = vif_window<9>(src, in.w, 2 * i, 2 * j, g);
    else if (scale == 2) v = vif_window<5>(src, in.w, 2 * i, 2 * j, g);
    else v = vif_window<3>(src, in.w, 2 * i, 2 * j, g);
    dst[(size_t)i * ow + j] = v;
}

// ---- 6: gradient magnitude similarity.  MS-GMSD works on 255 * image with t = 170 and alpha = 0.5; GMSD on the once-pooled
// [0, 1] image with t = 170 / 255^2 (scale 1 of the same chain)
__global__ __launch_bounds__(NT) void gms_kernel(ScaleSet S)
{
    const int s = blockIdx.z, b = blockIdx.y, tile = blockIdx.x;
    if (tile >= S.ntiles[s]) return;
    const Plane P = S.p[s];
    const int j = (tile % S.tiles_x[s]) * TW + threadIdx.x, i = (tile / S.tiles_x[s]) * TH + threadIdx.y;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < P.h && j < P.w) {
        float nx[9], ny[9];
        load3x3(P.x + (size_t)b * P.h * P.w, P.h, P.w, i, j, nx);
        load3x3(P.y + (size_t)b * P.h * P.w, P.h, P.w, i, j, ny);
        const float gx = grad9(nx), gy = grad9(ny);
        const float a = 255.f * gx, c = 255.f * gy, alpha = 0.5f, t = 170.f;
        const float g = ((2.f - alpha) * a * c + t) / (a * a + c * c - alpha * a * c + t);
        acc[0] = g;
        acc[1] = (double)g * g;
        if (s == 1) {
            const float t1 = 170.f / 65025.f;
            const float g1 = (2.f * gx * gy + t1) / (gx * gx + gy * gy + t1);
            acc[2] = g1;
            acc[3] = (double)g1 * g1;
        }
    }
    block_partials<4>(acc, S.part[s] + ((size_t)b * S.ntiles[s] + tile) * 4);
}

// ---- 7: HaarPSI on P = 255 * U1.  Scale s has k = 2^(s+1): rows i - k/2 + 1 .. i + k/2, the upper half +1/k, the lower half -1/k
// (and the transpose); all three windows lie in the 8 x 8 neighbourhood rows i-3 .. i+4.  A workgroup stages its 64 x 4 tile with
// that halo ((4 + 7) x (64 + 7) pixels per image, zero outside the image = the padding) in LDS once.
constexpr int HROWS = TH + 7, HCOLS = TW + 7, HSTRIDE = TW + 8;

__device__ __forceinline__ void haar_stage(const float* __restrict__ p, int h, int w, int i0, int j0, float* __restrict__ s)
{
    for (int k = threadIdx.y * TW + threadIdx.x; k < HROWS * HCOLS; k += NT) {
        const int r = k / HCOLS, c = k % HCOLS;
        s[r * HSTRIDE + c] = 255.f * ldz(p, h, w, i0 - 3 + r, j0 - 3 + c);
    }
}

// s: the staged tile at this thread's neighbourhood corner (row i - 3, column j - 3)
__device__ __forceinline__ void haar_coeffs(const float* __restrict__ s, float (&c)[3][2])
{
    float q[3][4] = {};       // per scale: top-left, top-right, bottom-left, bottom-right sums
#pragma unroll
    for (int dr = -3; dr <= 4; ++dr)
#pragma unroll
        for (int dc = -3; dc <= 4; ++dc) {
            const float v = s[(dr + 3) * HSTRIDE + dc + 3];
            const int quad = (dr > 0 ? 2 : 0) + (dc > 0 ? 1 : 0);
            q[2][quad] += v;
            if (dr >= -1 && dr <= 2 && dc >= -1 && dc <= 2) q[1][quad] += v;
            if (dr >= 0 && dr <= 1 && dc >= 0 && dc <= 1) q[0][quad] += v;
        }
#pragma unroll
    for (int sc = 0; sc < 3; ++sc) {
        const float inv = 1.f / (float)(2 << sc);
        c[sc][0] = fabsf(((q[sc][0] + q[sc][1]) - (q[sc][2] + q[sc][3])) * inv);
        c[sc][1] = fabsf(((q[sc][0] + q[sc][2]) - (q[sc][1] + q[sc][3])) * inv);
    }
}

__global__ __launch_bounds__(NT) void haarpsi_kernel(Plane P, double* __restrict__ part, int tiles_x, int ntiles)
{
    __shared__ float sx[HROWS * HSTRIDE], sy[HROWS * HSTRIDE];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int j0 = (tile % tiles_x) * TW, i0 = (tile / tiles_x) * TH;
    const int j = j0 + threadIdx.x, i = i0 + threadIdx.y;
    haar_stage(P.x + (size_t)b * P.h * P.w, P.h, P.w, i0, j0, sx);
    haar_stage(P.y + (size_t)b * P.h * P.w, P.h, P.w, i0, j0, sy);
    __syncthreads();
    double acc[2] = {0.0, 0.0};
    if (i < P.h && j < P.w) {
        float cx[3][2], cy[3][2];
        haar_coeffs(sx + threadIdx.y * HSTRIDE + threadIdx.x, cx);
        haar_coeffs(sy + threadIdx.y * HSTRIDE + threadIdx.x, cy);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const float wgt = fmaxf(cx[2][o], cy[2][o]) + (cx[2][o] - cx[2][o]) + (cy[2][o] - cy[2][o]);   // fmaxf drops a NaN: put it back
            const float sm = (simf(cx[0][o], cy[0][o], 30.f) + simf(cx[1][o], cy[1][o], 30.f)) * 0.5f;
            const float sg = 1.f / (1.f + expf(-4.2f * sm));
            acc[0] += (double)(sg * wgt);
            acc[1] += (double)wgt;
        }
    }
    block_partials<2>(acc, part + ((size_t)b * ntiles + tile) * 2);
}

// ---- 8-9: MDSI on the pooled [0, 1] image m: L = 0.9999 * 255 m, H = -0.01 * 255 m, M = -0.09 * 255 m (a grey image repeated to RGB)
__device__ __forceinline__ void mdsi_z(const float* __restrict__ px, const float* __restrict__ py, int h, int w, int i, int j, float& re, float& im)
{
    float nx[9], ny[9], na[9];
    load3x3(px, h, w, i, j, nx);
    load3x3(py, h, w, i, j, ny);
    const float vx = 255.f * nx[4], vy = 255.f * ny[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        nx[k] = 0.9999f * (255.f * nx[k]);
        ny[k] = 0.9999f * (255.f * ny[k]);
        na[k] = (nx[k] + ny[k]) * 0.5f;
    }
    const float gx = grad9(nx), gy = grad9(ny), ga = grad9(na);
    const float gs = simf(gx, gy, 140.f) + simf(gx, ga, 55.f) - simf(gy, ga, 55.f);
    const float hx = -0.01f * vx, hy = -0.01f * vy, mx = -0.09f * vx, my = -0.09f * vy;
    const float cs = (2.f * (hx * hy + mx * my) + 550.f) / (hx * hx + hy * hy + mx * mx + my * my + 550.f);
    const float g = 0.6f * gs + (1.f - 0.6f) * cs;
    const float mag = sqrtf(sqrtf(fabsf(g)));              // |G|^0.25
    if (g < 0.f) {                                         // the complex power's argument: q * pi
        re = mag * 0.70710678118654752f;
        im = mag * 0.70710678118654752f;
    } else {
        re = mag;
        im = mag * 0.f;                                    // keeps a NaN / inf visible in both parts, as cos / sin of the product do
    }
}

__global__ __launch_bounds__(NT) void mdsi_kernel(Plane P, const double* __restrict__ pass1, double* __restrict__ part, int tiles_x, int ntiles, int second)
{
    const int b = blockIdx.y, tile = blockIdx.x;
    const int j = (tile % tiles_x) * TW + threadIdx.x, i = (tile / tiles_x) * TH + threadIdx.y;
    double mre = 0.0, mim = 0.0;
    if (second) {
        const double n = (double)P.h * (double)P.w;
        mre = image_sum(pass1 + (size_t)b * ntiles * 2, ntiles, 2, 0) / n;
        mim = image_sum(pass1 + (size_t)b * ntiles * 2, ntiles, 2, 1) / n;
    }
    double acc[2] = {0.0, 0.0};
    if (i < P.h && j < P.w) {
        float re, im;
        mdsi_z(P.x + (size_t)b * P.h * P.w, P.y + (size_t)b * P.h * P.w, P.h, P.w, i, j, re, im);
        if (second) {
            const double dr = (double)re - mre, di = (double)im - mim;
            acc[0] = sqrt(dr * dr + di * di);
        } else {
            acc[0] = re;
            acc[1] = im;
        }
    }
    if (second) {
        const double one[1] = {acc[0]};
        block_partials<1>(one, part + ((size_t)b * ntiles + tile));
    } else {
        block_partials<2>(acc, part + ((size_t)b * ntiles + tile) * 2);
    }
}

// ---- 10: VIF's per-scale statistics over valid N x N windows, one workgroup per 16 x 16 windows.  The (16 + N - 1)^2 pixels under them
// go to LDS once; the Gaussian is the outer product of its 1-D form, so the statistics are one horizontal pass into LDS and one
// vertical pass per window.
// Variances and the covariance are taken in two stages, each about the value at the centre of its own window, never as E[x^2] - mu^2
// of the raw values (as ssim_kernel of loss_kernels.hip): per row the moments of x - (the row window's centre pixel), then down the
// column the mean of the row variances plus the variance of the row means about the centre row's mean (var = E[var_row] +
// Var[mean_row]).  Every subtraction is between neighbours, so a window over a flat region has variance and covariance exactly 0
// whatever its level (the zero background of an XMM frame).  An origin shared by the whole tile (its first pixel, as this kernel had
// it) left (x - origin)^2 * 1e-7 of rounding in every window away from that value: with a source on a tile's first pixel and zero
// background under the rest, 2e-8 per window, all of one sign -- 7e-5 to 9e-5 of the two sums of an 80 x 80 image, 4.7 times the bar.
constexpr int VT = 16;                   // windows per tile side
constexpr int VIN = VT + 17 - 1;         // largest pixel tile side (17 taps)
constexpr int VSTRIDE = VIN + 1;         // row stride in LDS: odd, so the horizontal pass's four rows per wave fall on different banks

// m = var t, var p, cov(t, p) of this thread's window
template <int N>
__device__ __forceinline__ void vif_tile(const float* __restrict__ t, const float* __restrict__ p, int h, int w, int i0, int j0,
                                         const float* __restrict__ g, float* __restrict__ sa, float* __restrict__ sc, float* __restrict__ hq,
                                         float (&m)[3])
{
    constexpr int IN = VT + N - 1, R = N / 2;
    const int tid = threadIdx.y * TW + threadIdx.x;
    for (int k = tid; k < IN * IN; k += NT) {
        const int r = k / IN, c = k % IN, ii = i0 + r, jj = j0 + c;
        const bool in = ii < h && jj < w;          // pixels past the image only feed windows that are not counted
        sa[r * VSTRIDE + c] = in ? t[(size_t)ii * w + jj] : 0.f;
        sc[r * VSTRIDE + c] = in ? p[(size_t)ii * w + jj] : 0.f;
    }
    __syncthreads();
    for (int k = tid; k < IN * VT; k += NT) {
        const int r = k / VT, c = k % VT;
        const float ca = sa[r * VSTRIDE + c + R], cq = sc[r * VSTRIDE + c + R];
        float rt = 0.f, rp = 0.f, rtt = 0.f, rpp = 0.f, rtp = 0.f;
#pragma unroll
        for (int dx = 0; dx < N; ++dx) {
            const float a = sa[r * VSTRIDE + c + dx] - ca, q = sc[r * VSTRIDE + c + dx] - cq, gw = g[dx];
            rt += gw * a;
            rp += gw * q;
            rtt += gw * (a * a);
            rpp += gw * (q * q);
            rtp += gw * (a * q);
        }
        hq[0 * VIN * VT + k] = ca + rt;            // row means
        hq[1 * VIN * VT + k] = cq + rp;
        hq[2 * VIN * VT + k] = rtt - rt * rt;      // row variances, row covariance
        hq[3 * VIN * VT + k] = rpp - rp * rp;
        hq[4 * VIN * VT + k] = rtp - rt * rp;
    }
    __syncthreads();
    const int ty = tid / VT, tx = tid % VT;
    const float qt = hq[0 * VIN * VT + (ty + R) * VT + tx], qp = hq[1 * VIN * VT + (ty + R) * VT + tx];
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, b4 = 0.f, wt = 0.f, wp = 0.f, wc = 0.f;
#pragma unroll
    for (int dy = 0; dy < N; ++dy) {
        const int at = (ty + dy) * VT + tx;
        const float gw = g[dy], et = hq[0 * VIN * VT + at] - qt, ep = hq[1 * VIN * VT + at] - qp;
        b0 += gw * et;
        b1 += gw * ep;
        b2 += gw * (et * et);
        b3 += gw * (ep * ep);
        b4 += gw * (et * ep);
        wt += gw * hq[2 * VIN * VT + at];
        wp += gw * hq[3 * VIN * VT + at];
        wc += gw * hq[4 * VIN * VT + at];
    }
    m[0] = wt + (b2 - b0 * b0);
    m[1] = wp + (b3 - b1 * b1);
    m[2] = wc + (b4 - b0 * b1);
}

// one window's two log10 terms from m = var t, var p, cov(t, p)
__device__ __forceinline__ void vif_terms(const float (&m)[3], double& num, double& den)
{
    const float eps = 1e-10f;
    float st = m[0], sp = m[1];
    st = st < 0.f ? 0.f : st;                  // clamp(min = 0) that keeps a NaN
    sp = sp < 0.f ? 0.f : sp;
    const float stp = m[2];
    float gg = stp / (st + eps);
    float sv = sp - gg * stp;
    if (st < eps) { gg = 0.f; sv = sp; st = 0.f; }
    if (sp < eps) { gg = 0.f; sv = 0.f; }
    if (gg < 0.f) { sv = sp; gg = 0.f; }
    sv = sv < eps ? eps : sv;
    const float inv_ln10 = 0.43429448190325176f;
    num = (double)(log1pf(gg * gg * st / (sv + 2.f)) * inv_ln10);      // log10(1 + x) without rounding 1 + x first
    den = (double)(log1pf(st / 2.f) * inv_ln10);
}

__global__ __launch_bounds__(NT) void vif_stats_kernel(ScaleSet S, VifWeights vw)
{
    __shared__ float sa[VIN * VSTRIDE], sc[VIN * VSTRIDE], hq[5 * VIN * VT];
    const int s = blockIdx.z, b = blockIdx.y, tile = blockIdx.x;
    if (tile >= S.ntiles[s]) return;
    const Plane P = S.p[s];
    const int n = 17 >> s | 1;                                 // 17, 9, 5, 3
    const int oh = P.h - n + 1, ow = P.w - n + 1;
    const int tid = threadIdx.y * TW + threadIdx.x;
    const int j0 = (tile % S.tiles_x[s]) * VT, i0 = (tile / S.tiles_x[s]) * VT;
    const float* g = vif_taps_to_lds(vw, s);
    const float* t = P.y + (size_t)b * P.h * P.w;              // y = target, x = preds
    const float* p = P.x + (size_t)b * P.h * P.w;
    float m[3];
    if (s == 0) vif_tile<17>(t, p, P.h, P.w, i0, j0, g, sa, sc, hq, m);
    else if (s == 1) vif_tile<9>(t, p, P.h, P.w, i0, j0, g, sa, sc, hq, m);
    else if (s == 2) vif_tile<5>(t, p, P.h, P.w, i0, j0, g, sa, sc, hq, m);
    else vif_tile<3>(t, p, P.h, P.w, i0, j0, g, sa, sc, hq, m);
    double acc[2] = {0.0, 0.0};
    if (i0 + tid / VT < oh && j0 + tid % VT < ow) vif_terms(m, acc[0], acc[1]);
    block_partials<2>(acc, S.part[s] + ((size_t)b * S.ntiles[s] + tile) * 2);
}

// ---- 11: one workgroup per image
__device__ __forceinline__ double pop_var(double s, double s2, double n)
{
    const double m = s / n, v = s2 / n - m * m;
    return v < 0.0 ? 0.0 : v;          // keeps a NaN
}

__global__ __launch_bounds__(NT) void finish_kernel(FinishArgs A, double* __restrict__ out)
{
    const int b = blockIdx.x;
    const double w[NSCALE] = {0.096, 0.596, 0.289, 0.019};
    double ms = 0.0, gmsd = 0.0, vnum = 0.0, vden = 0.0;
    for (int s = 0; s < NSCALE; ++s) {
        const double* gp = A.gms[s] + (size_t)b * A.gms_tiles[s] * 4;
        const double s1 = image_sum(gp, A.gms_tiles[s], 4, 0), s2 = image_sum(gp, A.gms_tiles[s], 4, 1);
        ms += w[s] * pop_var(s1, s2, A.gms_count[s]);
        if (s == 1) {
            const double t1 = image_sum(gp, A.gms_tiles[s], 4, 2), t2 = image_sum(gp, A.gms_tiles[s], 4, 3);
            gmsd = sqrt(pop_var(t1, t2, A.gms_count[s]));
        }
        const double* vp = A.vif[s] + (size_t)b * A.vif_tiles[s] * 2;
        vnum += image_sum(vp, A.vif_tiles[s], 2, 0);
        vden += image_sum(vp, A.vif_tiles[s], 2, 1);
    }
    const double* hp = A.haar + (size_t)b * A.haar_tiles * 2;
    const double hn = image_sum(hp, A.haar_tiles, 2, 0), hd = image_sum(hp, A.haar_tiles, 2, 1);
    const double dev = image_sum(A.mdsi2 + (size_t)b * A.mdsi_tiles, A.mdsi_tiles, 1, 0);
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const double eps = 1.1920928955078125e-07;       // fp32 machine epsilon
        const double v = (hn + eps) / (hd + eps), l = log(v / (1.0 - v)) / 4.2;
        double* o = out + (size_t)b * XSD_EXTM_OUT;
        o[0] = gmsd;
        o[1] = sqrt(ms);
        o[2] = l * l;
        o[3] = sqrt(sqrt(dev / A.mdsi_count));           // (mean deviation)^(o / rho), o = 0.25, rho = 1
        o[4] = vnum;
        o[5] = vden;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int pool2_dim(int n, int d) { return (n + d) / 2; }
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- geometry and workspace layout of one (B, H, W): computed in one place, for xsd_ext_metrics_eval and xsd_ext_metrics_test_stage
struct ExtLayout {
    PoolDims pd;
    int mk, mh, mw;                                  // MDSI: kernel size, pooled dims
    int vh[NSCALE], vw[NSCALE];                      // VIF chain: image dims per scale ([0] = H, W)
    int gh[NSCALE], gw[NSCALE];                      // gradient-magnitude chain: H x W, then U1..U3
    int g_tx[NSCALE], g_nt[NSCALE], v_tx[NSCALE], v_nt[NSCALE];
    int h_tx, h_nt, m_tx, m_nt;
    size_t o_gms[NSCALE], o_vif[NSCALE], o_haar, o_md1, o_md2;       // doubles (tile partials) first
    size_t o_ux, o_uy, o_mx, o_my, o_vx[NSCALE], o_vy[NSCALE];       // then the float images ([0] of o_vx / o_vy unused)
    size_t u_off[NSCALE];                            // float offset of U1..U3 inside o_ux / o_uy ([0] unused)
    size_t bytes;
};

ExtLayout ext_layout(int B, int H, int W)
{
    ExtLayout L;
    PoolDims& pd = L.pd;
    pd.H = H; pd.W = W;
    int d = std::max(H % 2, W % 2);
    pd.h1 = pool2_dim(H, d); pd.w1 = pool2_dim(W, d);
    d = std::max(pd.h1 % 2, pd.w1 % 2);
    pd.h2 = pool2_dim(pd.h1, d); pd.w2 = pool2_dim(pd.w1, d);
    d = std::max(pd.h2 % 2, pd.w2 % 2);
    pd.h3 = pool2_dim(pd.h2, d); pd.w3 = pool2_dim(pd.w2, d);
    L.mk = std::max(1, (int)std::nearbyint((double)std::min(H, W) / 256.0));      // Python's round: ties to even
    L.mh = (H - 1) / L.mk + 1; L.mw = (W - 1) / L.mk + 1;
    L.vh[0] = H; L.vw[0] = W;
    for (int s = 1; s < NSCALE; ++s) {
        L.vh[s] = (L.vh[s - 1] - VIF_TAPS[s] + 2) / 2;
        L.vw[s] = (L.vw[s - 1] - VIF_TAPS[s] + 2) / 2;
    }
    const int gh[NSCALE] = {H, pd.h1, pd.h2, pd.h3}, gw[NSCALE] = {W, pd.w1, pd.w2, pd.w3};

    // ---- workspace: doubles (tile partials) first, then the float images
    const size_t nB = (size_t)B;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    for (int s = 0; s < NSCALE; ++s) {
        L.gh[s] = gh[s]; L.gw[s] = gw[s];
        L.g_tx[s] = cdiv(gw[s], TW); L.g_nt[s] = L.g_tx[s] * cdiv(gh[s], TH);
        L.v_tx[s] = cdiv(L.vw[s] - VIF_TAPS[s] + 1, VT); L.v_nt[s] = L.v_tx[s] * cdiv(L.vh[s] - VIF_TAPS[s] + 1, VT);
        L.o_gms[s] = take(nB * L.g_nt[s] * 4 * sizeof(double));
        L.o_vif[s] = take(nB * L.v_nt[s] * 2 * sizeof(double));
    }
    L.h_tx = L.g_tx[1]; L.h_nt = L.g_nt[1];
    L.m_tx = cdiv(L.mw, TW); L.m_nt = L.m_tx * cdiv(L.mh, TH);
    L.o_haar = take(nB * L.h_nt * 2 * sizeof(double));
    L.o_md1 = take(nB * L.m_nt * 2 * sizeof(double));
    L.o_md2 = take(nB * L.m_nt * sizeof(double));
    const size_t n_u = (size_t)pd.h1 * pd.w1 + (size_t)pd.h2 * pd.w2 + (size_t)pd.h3 * pd.w3;
    L.o_ux = take(nB * n_u * sizeof(float)); L.o_uy = take(nB * n_u * sizeof(float));
    L.o_mx = take(nB * L.mh * L.mw * sizeof(float)); L.o_my = take(nB * L.mh * L.mw * sizeof(float));
    L.o_vx[0] = L.o_vy[0] = 0;
    for (int s = 1; s < NSCALE; ++s) {
        L.o_vx[s] = take(nB * L.vh[s] * L.vw[s] * sizeof(float));
        L.o_vy[s] = take(nB * L.vh[s] * L.vw[s] * sizeof(float));
    }
    L.u_off[0] = 0; L.u_off[1] = 0; L.u_off[2] = nB * pd.h1 * pd.w1;
    L.u_off[3] = nB * ((size_t)pd.h1 * pd.w1 + (size_t)pd.h2 * pd.w2);
    L.bytes = off;
    return L;
}

}   // namespace

struct xsd_ext_metrics {
    void* ws = nullptr;
    size_t ws_bytes = 0;
    int B = 0, H = 0, W = 0;          // the last xsd_ext_metrics_eval that was enqueued (0: none yet)
};

int xsd_ext_metrics_create(xsd_ext_metrics** out)
{
    if (!out) return fail(XSD_ERR_ARG, "xsd_ext_metrics_create: null output pointer");
    xsd_ext_metrics* m = new (std::nothrow) xsd_ext_metrics();
    if (!m) return fail(XSD_ERR_NOMEM, "out of host memory");
    *out = m;
    return XSD_OK;
}

void xsd_ext_metrics_destroy(xsd_ext_metrics* m)
{
    if (!m) return;
    xsd::dev_free(m->ws);
    delete m;
}

#define EXTM_HIPCHK(expr)                                                                                                      \
    do {                                                                                                                       \
        hipError_t _e = (expr);                                                                                                \
        if (_e != hipSuccess) return fail(XSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

int xsd_ext_metrics_eval(xsd_ext_metrics* m, const float* dev_preds, const float* dev_target, double* dev_out, int B, int H, int W, void* stream)
{
    if (!m || !dev_preds || !dev_target || !dev_out) return fail(XSD_ERR_ARG, "xsd_ext_metrics_eval: null pointer");
    if (B < 1 || B > 65535) return fail(XSD_ERR_ARG, "xsd_ext_metrics_eval: B must be 1..65535 (got %d)", B);
    if (H < 41 || W < 41 || H > 16384 || W > 16384)
        return fail(XSD_ERR_ARG, "xsd_ext_metrics_eval: H and W must be 41..16384 (got %d x %d): vif_p's 17-tap valid filter over four scales "
                                 "needs at least 41 pixels", H, W);
    hipStream_t st = (hipStream_t)stream;

    m->B = 0;                                      // nothing to read back until this eval is enqueued whole
    const ExtLayout L = ext_layout(B, H, W);
    const PoolDims& pd = L.pd;
    const int mk = L.mk, mh = L.mh, mw = L.mw, h_tx = L.h_tx, h_nt = L.h_nt, m_tx = L.m_tx, m_nt = L.m_nt;
    const int *vh = L.vh, *vw_ = L.vw, *gh = L.gh, *gw = L.gw, *g_tx = L.g_tx, *g_nt = L.g_nt, *v_tx = L.v_tx, *v_nt = L.v_nt;
    const size_t *o_gms = L.o_gms, *o_vif = L.o_vif, *o_vx = L.o_vx, *o_vy = L.o_vy, *u_off = L.u_off;
    const size_t o_haar = L.o_haar, o_md1 = L.o_md1, o_md2 = L.o_md2, o_ux = L.o_ux, o_uy = L.o_uy, o_mx = L.o_mx, o_my = L.o_my;
    if (L.bytes > m->ws_bytes) {
        EXTM_HIPCHK(hipStreamSynchronize(st));
        if (m->ws) EXTM_HIPCHK(xsd::dev_free(m->ws));
        m->ws = nullptr; m->ws_bytes = 0; m->B = 0;
        if (xsd::dev_alloc(&m->ws, L.bytes) != hipSuccess)
            return fail(XSD_ERR_NOMEM, "xsd_ext_metrics_eval: workspace allocation of %zu bytes failed", L.bytes);
        m->ws_bytes = L.bytes;
    }
    char* ws = (char*)m->ws;
    auto F = [&](size_t o) { return (float*)(ws + o); };
    auto D = [&](size_t o) { return (double*)(ws + o); };

    VifWeights vw;
    for (int s = 0; s < NSCALE; ++s) {
        const int n = VIF_TAPS[s];
        const double sigma = n / 3.0;
        double g[17], sum = 0.0;
        for (int k = 0; k < n; ++k) { const double c = k - n / 2; g[k] = std::exp(-c * c / (2.0 * sigma * sigma)); sum += g[k]; }
        for (int k = 0; k < 17; ++k) vw.g[s][k] = k < n ? (float)(g[k] / sum) : 0.f;
    }

    const dim3 blk(TW, TH);
    // 1: pool chain
    {
        const int cx = cdiv(pd.w1, 4), cy = cdiv(pd.h1, 4), tx = cdiv(cx, TW);
        hipLaunchKernelGGL(pool_chain_kernel, dim3(tx * cdiv(cy, TH), B, 2), blk, 0, st, dev_preds, dev_target, F(o_ux), F(o_uy), pd, cx, tx);
    }
    // 2: MDSI pooling
    hipLaunchKernelGGL(mdsi_pool_kernel, dim3(m_nt, B, 2), blk, 0, st, dev_preds, dev_target, F(o_mx), F(o_my), H, W, mh, mw, mk, m_tx);
    // 3-5: VIF chain
    for (int s = 1; s < NSCALE; ++s) {
        Plane in;
        in.x = s == 1 ? dev_preds : F(o_vx[s - 1]);
        in.y = s == 1 ? dev_target : F(o_vy[s - 1]);
        in.h = vh[s - 1]; in.w = vw_[s - 1];
        const int tx = cdiv(vw_[s], TW);
        hipLaunchKernelGGL(vif_decimate_kernel, dim3(tx * cdiv(vh[s], TH), B, 2), blk, 0, st, in, F(o_vx[s]), F(o_vy[s]), vh[s], vw_[s], s, vw, tx);
    }
    // 6: gradient magnitude similarity, four scales
    ScaleSet G, V;
    int g_max = 0, v_max = 0;
    for (int s = 0; s < NSCALE; ++s) {
        G.p[s].x = s == 0 ? dev_preds : F(o_ux) + u_off[s];
        G.p[s].y = s == 0 ? dev_target : F(o_uy) + u_off[s];
        G.p[s].h = gh[s]; G.p[s].w = gw[s];
        G.part[s] = D(o_gms[s]); G.tiles_x[s] = g_tx[s]; G.ntiles[s] = g_nt[s];
        g_max = std::max(g_max, g_nt[s]);
        V.p[s].x = s == 0 ? dev_preds : F(o_vx[s]);
        V.p[s].y = s == 0 ? dev_target : F(o_vy[s]);
        V.p[s].h = vh[s]; V.p[s].w = vw_[s];
        V.part[s] = D(o_vif[s]); V.tiles_x[s] = v_tx[s]; V.ntiles[s] = v_nt[s];
        v_max = std::max(v_max, v_nt[s]);
    }
    hipLaunchKernelGGL(gms_kernel, dim3(g_max, B, NSCALE), blk, 0, st, G);
    // 7: HaarPSI on the once-pooled image
    hipLaunchKernelGGL(haarpsi_kernel, dim3(h_nt, B), blk, 0, st, G.p[1], D(o_haar), h_tx, h_nt);
    // 8-9: MDSI
    Plane M;
    M.x = F(o_mx); M.y = F(o_my); M.h = mh; M.w = mw;
    hipLaunchKernelGGL(mdsi_kernel, dim3(m_nt, B), blk, 0, st, M, (const double*)nullptr, D(o_md1), m_tx, m_nt, 0);
    hipLaunchKernelGGL(mdsi_kernel, dim3(m_nt, B), blk, 0, st, M, (const double*)D(o_md1), D(o_md2), m_tx, m_nt, 1);
    // 10: VIF statistics, four scales
    hipLaunchKernelGGL(vif_stats_kernel, dim3(v_max, B, NSCALE), blk, 0, st, V, vw);
    // 11: finish
    FinishArgs A;
    for (int s = 0; s < NSCALE; ++s) {
        A.gms[s] = D(o_gms[s]); A.vif[s] = D(o_vif[s]);
        A.gms_tiles[s] = g_nt[s]; A.vif_tiles[s] = v_nt[s];
        A.gms_count[s] = (double)gh[s] * (double)gw[s];
    }
    A.haar = D(o_haar); A.mdsi2 = D(o_md2);
    A.haar_tiles = h_nt; A.mdsi_tiles = m_nt;
    A.mdsi_count = (double)mh * (double)mw;
    hipLaunchKernelGGL(finish_kernel, dim3(B), blk, 0, st, A, dev_out);
    EXTM_HIPCHK(hipGetLastError());
    m->B = B; m->H = H; m->W = W;
    return XSD_OK;
}

int xsd_ext_metrics_test_stage(xsd_ext_metrics* m, int stage, int side, void* dev_dst, int64_t dst_bytes, int* info, void* stream)
{
    if (!m || !dev_dst || !info) return fail(XSD_ERR_ARG, "xsd_ext_metrics_test_stage: null pointer");
    if (stage < 0 || stage >= XSD_EXTM_STAGES) return fail(XSD_ERR_ARG, "xsd_ext_metrics_test_stage: unknown stage %d (0..%d)", stage, XSD_EXTM_STAGES - 1);
    if (side != 0 && side != 1) return fail(XSD_ERR_ARG, "xsd_ext_metrics_test_stage: side must be 0 (preds) or 1 (target), got %d", side);
    if (!m->B || !m->ws) return fail(XSD_ERR_ARG, "xsd_ext_metrics_test_stage: this handle has not evaluated anything yet");
    const ExtLayout L = ext_layout(m->B, m->H, m->W);
    const size_t nB = (size_t)m->B;
    size_t off = 0, bytes = 0;
    int h = 0, w = 0, entries = 0, tx = 0, nt = 0, th = TH, tw = TW;
    if (stage <= XSD_EXTM_STAGE_U3) {                        // U1..U3
        const int s = stage - XSD_EXTM_STAGE_U1 + 1;
        h = L.gh[s]; w = L.gw[s];
        off = (side ? L.o_uy : L.o_ux) + L.u_off[s] * sizeof(float);
    } else if (stage == XSD_EXTM_STAGE_M) {
        h = L.mh; w = L.mw;
        off = side ? L.o_my : L.o_mx;
    } else if (stage <= XSD_EXTM_STAGE_V3) {                 // V1..V3
        const int s = stage - XSD_EXTM_STAGE_V1 + 1;
        h = L.vh[s]; w = L.vw[s];
        off = side ? L.o_vy[s] : L.o_vx[s];
    } else if (stage <= XSD_EXTM_STAGE_GMS3) {
        const int s = stage - XSD_EXTM_STAGE_GMS0;
        h = L.gh[s]; w = L.gw[s]; entries = 4; tx = L.g_tx[s]; nt = L.g_nt[s]; off = L.o_gms[s];
    } else if (stage == XSD_EXTM_STAGE_HAAR) {
        h = L.gh[1]; w = L.gw[1]; entries = 2; tx = L.h_tx; nt = L.h_nt; off = L.o_haar;
    } else if (stage == XSD_EXTM_STAGE_MDSI1 || stage == XSD_EXTM_STAGE_MDSI2) {
        const bool first = stage == XSD_EXTM_STAGE_MDSI1;
        h = L.mh; w = L.mw; entries = first ? 2 : 1; tx = L.m_tx; nt = L.m_nt; off = first ? L.o_md1 : L.o_md2;
    } else {
        const int s = stage - XSD_EXTM_STAGE_VIF0;
        h = L.vh[s] - VIF_TAPS[s] + 1; w = L.vw[s] - VIF_TAPS[s] + 1;       // windows, not pixels
        entries = 2; tx = L.v_tx[s]; nt = L.v_nt[s]; off = L.o_vif[s]; th = VT; tw = VT;
    }
    bytes = entries ? nB * nt * entries * sizeof(double) : nB * h * w * sizeof(float);
    info[0] = m->B; info[1] = h; info[2] = w; info[3] = entries;
    info[4] = entries ? tx : 0; info[5] = entries ? nt : 0; info[6] = entries ? th : 0; info[7] = entries ? tw : 0;
    if (dst_bytes < 0 || (size_t)dst_bytes < bytes)
        return fail(XSD_ERR_ARG, "xsd_ext_metrics_test_stage: buffer too small for stage %d: %lld bytes given, %zu needed", stage, (long long)dst_bytes, bytes);
    if (off + bytes > m->ws_bytes) return fail(XSD_ERR_ARG, "xsd_ext_metrics_test_stage: the region lies outside the workspace");
    EXTM_HIPCHK(hipMemcpyAsync(dev_dst, (const char*)m->ws + off, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return XSD_OK;
}
