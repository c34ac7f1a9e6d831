// fsim.hip -- the sixth extended test metric of the reference (metrics/xmm_metric_collection.py:41-61): piq 0.7.x
// fsim(x, y, chromatic=False) with every default, on single-channel [0, 1] images.  The formulas are restated from piq's published
// code (include/xsd.h; tests/golden/fsim_torch.py): parity with piq itself is unpinned.
//
// The images are pooled to h x w (a few hundred a side, often prime: 832 -> 277).  Phase congruency needs fft2 of the pooled image and
// ifft2 of its product with each of 16 log-Gabor filters.  No factorisation: a 1-D pass is a dense product with the n x n DFT matrix,
// one complex GEMM kernel (64 x 64 tile per workgroup, K in steps of 16 through LDS, 4 x 4 complex accumulators per thread in double;
// blockIdx.z = image x filter).  What depends on (h, w) only -- the DFT matrices, the filters, the noise constants -- is a plan.
//
// One xsd_fsim_eval is a fixed chain of 9 launches, whatever B is (s = 0 preds, 1 target; sb = s * B + image):
//   1  pool          x, y -> 255 * the ks x ks mean (double)
//   2  cgemm         rows forward:      Y = P * Ww                                      2B products
//   3  cgemm         columns forward:   F = Wh * Y
//   4  cgemm         columns inverse:   Z[f] = conj(Wh) * (F . filt[f])                 32B products; the filtered spectra are never stored
//   5  cgemm         rows inverse:      eo[f] = Z[f] * conj(Ww) / (h w)  -> fp32
//   6  pc_point      per (sb, orientation, pixel): sum of |eo| over the scales, the energy before its threshold, |eo[o, 0]|^2
//   7  median_T      per (sb, orientation): exact median by radix select -> the noise threshold T
//   8  fsim_map      per pixel: pc of both images, Scharr gradients, the similarity product -> per-tile sums
//   9  finish        one workgroup per image: tile sums -> fsim
// Responses are stored fp32; every other map and every sum is double.  Every workgroup reduces its tile in a fixed order into its own
// slot; `finish` adds an image's slots in a fixed order.  No float atomics: an image's value does not depend on its batch-mates or on
// the run, and a NaN stays in its image (the GEMM's batches never mix; out-of-range tile elements are zeros).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "../../include/xsd.h"

#include "xsd_err.h"
#include "xsd_mem.h"
#define fail xsd::failf      // the thread-local message of xsd_last_error()

namespace {

constexpr int TW = 64, TH = 4, NT = TW * TH;      // pointwise kernels: one workgroup = a 64 x 4 tile of a map = four waves
constexpr int NO = 4, NS = 4, NF = NO * NS;       // orientations, scales, filters (index o * NS + s)
constexpr int MAX_SIDE = 1024;
constexpr double PI = 3.14159265358979323846;

// ---- the complex GEMM:  C[bt][m][n] = scale * sum_k A[bt][m][k] * B[bt][k][n]
enum { K_CF32 = 1, K_CF64 = 2, K_RF64 = 3 };

struct Opnd {             // element (r, c) of batch bt = p[(bt / bdiv) * bstride + r * ld + c] (conjugated if conj), times
    const void* p;        // filt[(bt % NF) * fstride + r * ld + c] if filt
    int kind, conj, bdiv;
    long long ld, bstride;
    const double* filt;
    long long fstride;
};

__device__ __forceinline__ double2 ld_op(const Opnd& o, int bt, int r, int c)
{
    const size_t at = (size_t)(bt / o.bdiv) * (size_t)o.bstride + (size_t)r * (size_t)o.ld + (size_t)c;
    double2 v;
    if (o.kind == K_CF64) {
        v = ((const double2*)o.p)[at];
    } else if (o.kind == K_CF32) {
        const float2 f = ((const float2*)o.p)[at];
        v = make_double2((double)f.x, (double)f.y);
    } else {
        v = make_double2(((const double*)o.p)[at], 0.0);
    }
    if (o.conj) v.y = -v.y;
    if (o.filt) {
        const double g = o.filt[(size_t)(bt % NF) * (size_t)o.fstride + (size_t)r * (size_t)o.ld + (size_t)c];
        v.x *= g;
        v.y *= g;
    }
    return v;
}

constexpr int GM = 64, GN = 64, GK = 16;

__global__ __launch_bounds__(256) void cgemm_kernel(Opnd A, Opnd Bo, void* __restrict__ C, int c_f32, double scale, int M, int N, int K)
{
    __shared__ double2 As[GK][GM + 1];        // [k][m]; + 1: the transposing writes of the k-contiguous loads spread over the banks
    __shared__ double2 Bs[GK][GN];            // [k][n]
    const int bt = blockIdx.z, m0 = blockIdx.y * GM, n0 = blockIdx.x * GN;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double2 acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < K; k0 += GK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            const int ka = e & 15, ma = e >> 4;
            As[ka][ma] = (m0 + ma < M && k0 + ka < K) ? ld_op(A, bt, m0 + ma, k0 + ka) : make_double2(0.0, 0.0);
            const int nb = e & 63, kb = e >> 6;
            Bs[kb][nb] = (k0 + kb < K && n0 + nb < N) ? ld_op(Bo, bt, k0 + kb, n0 + nb) : make_double2(0.0, 0.0);
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; ++kk) {
            double2 a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = As[kk][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = Bs[kk][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc[r][c].x = fma(a[r].x, b[c].x, acc[r][c].x);
                    acc[r][c].x = fma(-a[r].y, b[c].y, acc[r][c].x);
                    acc[r][c].y = fma(a[r].x, b[c].y, acc[r][c].y);
                    acc[r][c].y = fma(a[r].y, b[c].x, acc[r][c].y);
                }
        }
        __syncthreads();
    }
    const size_t base = (size_t)bt * (size_t)M * (size_t)N;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = m0 + ty + 16 * r, n = n0 + tx + 16 * c;
            if (m < M && n < N) {
                const size_t at = base + (size_t)m * N + n;
                if (c_f32) ((float2*)C)[at] = make_float2((float)(acc[r][c].x * scale), (float)(acc[r][c].y * scale));
                else ((double2*)C)[at] = make_double2(acc[r][c].x * scale, acc[r][c].y * scale);
            }
        }
}

// ---- fixed-order reductions (as in ext_metrics.hip)
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

// ---- 1: 255 * x, then the ks x ks mean without padding (the remainder is dropped): every tap is inside H x W
__global__ __launch_bounds__(NT) void pool_kernel(const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ pooled, int B,
                                                  int H, int W, int h, int w, int ks, int tiles_x)
{
    const int sb = blockIdx.y, b = sb % B;
    const float* src = (sb >= B ? y : x) + (size_t)b * H * W;
    const int j = (blockIdx.x % tiles_x) * TW + threadIdx.x, i = (blockIdx.x / tiles_x) * TH + threadIdx.y;
    if (i >= h || j >= w) return;
    double s = 0.0;
    for (int a = 0; a < ks; ++a)
        for (int c = 0; c < ks; ++c) s += (double)src[(size_t)(i * ks + a) * W + (j * ks + c)] * 255.0;
    pooled[(size_t)sb * h * w + (size_t)i * w + j] = s / (double)(ks * ks);
}

// ---- 6: per (sb, orientation, pixel)
__global__ __launch_bounds__(NT) void pc_point_kernel(const float2* __restrict__ eo, double* __restrict__ en, double* __restrict__ an,
                                                      float* __restrict__ a0sq, int hw)
{
    const int sb = blockIdx.y, o = blockIdx.z;
    const int pix = blockIdx.x * NT + threadIdx.y * TW + threadIdx.x;
    if (pix >= hw) return;
    const float2* src = eo + ((size_t)sb * NF + (size_t)o * NS) * hw + pix;
    double e[NS], d[NS], sum_an = 0.0, sum_e = 0.0, sum_o = 0.0, a0 = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float2 v = src[(size_t)s * hw];
        e[s] = v.x;
        d[s] = v.y;
        const double a = sqrt(e[s] * e[s] + d[s] * d[s]);
        if (s == 0) a0 = a;
        sum_an += a;
        sum_e += e[s];
        sum_o += d[s];
    }
    const double xe = sqrt(sum_e * sum_e + sum_o * sum_o) + 2.220446049250313e-16;       // the eps of the yardstick's dtype
    const double me = sum_e / xe, mo = sum_o / xe;
    double energy = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) energy += e[s] * me + d[s] * mo - fabs(e[s] * mo - d[s] * me);
    const size_t at = ((size_t)sb * NO + o) * hw + pix;
    en[at] = energy;
    an[at] = sum_an;
    a0sq[at] = (float)(a0 * a0);
}

// ---- 7: the element torch.median picks: rank (n - 1) / 2 of the row in ascending order, by a 4 x 8 bit radix select on keys that
// order like the floats (integer histograms in LDS); NaN if the row holds one.  Every thread of the workgroup returns the value.
constexpr int MED_NT = 1024;          // one workgroup per row: few rows (8 B), long rows (h w)
__device__ __forceinline__ unsigned f2key(unsigned bits) { return (bits >> 31) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ unsigned key2f(unsigned key) { return (key >> 31) ? (key & 0x7fffffffu) : ~key; }

__device__ __forceinline__ float select_median(const float* __restrict__ row, int n)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_rank, s_nan;
    const int tid = threadIdx.x, nt = blockDim.x;
    const unsigned* bits = (const unsigned*)row;
    if (tid == 0) { s_prefix = 0u; s_rank = (unsigned)((n - 1) / 2); s_nan = 0u; }
    unsigned mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int k = tid; k < 256; k += nt) hist[k] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix;
        unsigned saw_nan = 0u;
        for (int i = tid; i < n; i += nt) {
            const unsigned u = bits[i];
            if (pass == 0 && (u & 0x7fffffffu) > 0x7f800000u) saw_nan = 1u;
            const unsigned key = f2key(u);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        if (saw_nan) s_nan = 1u;
        __syncthreads();
        if (tid == 0) {
            unsigned rank = s_rank, cum = 0u;
            int bin = 0;
            for (; bin < 255; ++bin) {
                if (cum + hist[bin] > rank) break;
                cum += hist[bin];
            }
            s_rank = rank - cum;
            s_prefix = prefix | ((unsigned)bin << shift);
        }
        mask |= 0xffu << shift;
        __syncthreads();
    }
    const unsigned out = s_nan ? 0x7fc00000u : key2f(s_prefix);
    return __uint_as_float(out);
}

__global__ __launch_bounds__(MED_NT) void median_kernel(const float* __restrict__ in, float* __restrict__ out, int n)
{
    const float v = select_median(in + (size_t)blockIdx.x * n, n);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

struct NoiseConsts {
    double em_n[NO], sum_an2[NO], sum_ai_aj[NO];
};

__global__ __launch_bounds__(MED_NT) void median_T_kernel(const float* __restrict__ a0sq, double* __restrict__ T, NoiseConsts nc, int hw)
{
    const int row = blockIdx.x, o = row % NO;             // row = sb * NO + o
    const double med = (double)select_median(a0sq + (size_t)row * hw, hw);
    if (threadIdx.x == 0) {
        const double mean_e2n = -med / log(0.5);
        const double noise_power = mean_e2n / nc.em_n[o];
        const double noise_energy2 = 2.0 * noise_power * nc.sum_an2[o] + 4.0 * noise_power * nc.sum_ai_aj[o];
        const double tau = sqrt(noise_energy2 / 2.0);
        T[row] = (tau * sqrt(PI / 2.0) + 2.0 * sqrt((2.0 - PI / 2.0) * tau * tau)) / 1.7;
    }
}

// ---- 8
__device__ __forceinline__ double ldz(const double* __restrict__ p, int h, int w, int i, int j)
{
    return (i >= 0 && i < h && j >= 0 && j < w) ? p[(size_t)i * w + j] : 0.0;
}

__device__ __forceinline__ double scharr(const double* __restrict__ p, int h, int w, int i, int j)
{
    double n[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) n[a * 3 + b] = ldz(p, h, w, i + a - 1, j + b - 1);
    const double gx = (3.0 * (n[2] - n[0]) + 10.0 * (n[5] - n[3]) + 3.0 * (n[8] - n[6])) / 16.0;
    const double gy = (3.0 * (n[6] - n[0]) + 10.0 * (n[7] - n[1]) + 3.0 * (n[8] - n[2])) / 16.0;
    return sqrt(gx * gx + gy * gy);
}

__device__ __forceinline__ double simd(double a, double b, double c) { return (2.0 * a * b + c) / (a * a + b * b + c); }

__device__ __forceinline__ double pc_of(const double* __restrict__ en, const double* __restrict__ an, const double* __restrict__ T, int sb,
                                        int hw, int pix)
{
    double es = 0.0, as = 0.0;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        const size_t at = ((size_t)sb * NO + o) * hw + pix;
        const double v = en[at] - T[sb * NO + o];
        es += v < 0.0 ? 0.0 : v;                   // max(., 0) that keeps a NaN
        as += an[at];
    }
    return es / as;
}

__global__ __launch_bounds__(NT) void fsim_map_kernel(const double* __restrict__ pooled, const double* __restrict__ en,
                                                      const double* __restrict__ an, const double* __restrict__ T, double* __restrict__ part,
                                                      int B, int h, int w, int tiles_x, int ntiles)
{
    const int b = blockIdx.y, tile = blockIdx.x;
    const int j = (tile % tiles_x) * TW + threadIdx.x, i = (tile / tiles_x) * TH + threadIdx.y;
    const int hw = h * w;
    double acc[2] = {0.0, 0.0};
    if (i < h && j < w) {
        const int pix = i * w + j;
        const double pcx = pc_of(en, an, T, b, hw, pix), pcy = pc_of(en, an, T, B + b, hw, pix);
        const double gx = scharr(pooled + (size_t)b * hw, h, w, i, j), gy = scharr(pooled + (size_t)(B + b) * hw, h, w, i, j);
        const double pcm = pcx > pcy ? pcx : pcy;
        acc[0] = simd(gx, gy, 160.0) * simd(pcx, pcy, 0.85) * pcm;
        acc[1] = pcm;
    }
    block_partials<2>(acc, part + ((size_t)b * ntiles + tile) * 2);
}

// ---- 9
__global__ __launch_bounds__(NT) void fsim_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int ntiles)
{
    const int b = blockIdx.x;
    const double* p = part + (size_t)b * ntiles * 2;
    const double num = image_sum(p, ntiles, 2, 0), den = image_sum(p, ntiles, 2, 1);
    if (threadIdx.x == 0 && threadIdx.y == 0) out[b] = num / den;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- the plan of one pooled size: everything that depends on (h, w) only, computed on the host in double
struct Plan {
    int h = 0, w = 0;
    double2* Wh = nullptr;        // h x h forward DFT matrix exp(-2 pi i (j k mod h) / h): symmetric, so also its own transpose
    double2* Ww = nullptr;        // w x w (the same allocation as Wh when h == w)
    double* filt = nullptr;       // [NF][h][w]
    NoiseConsts nc;
    unsigned long long stamp = 0;
};

void free_plan(Plan& p)
{
    if (p.Ww && p.Ww != p.Wh) xsd::dev_free(p.Ww);
    if (p.Wh) xsd::dev_free(p.Wh);
    if (p.filt) xsd::dev_free(p.filt);
    p = Plan();
}

void dft_matrix(int n, std::vector<double2>& m)
{
    std::vector<double2> tw(n);
    for (int r = 0; r < n; ++r) {
        const double a = -2.0 * PI * (double)r / (double)n;
        tw[r] = make_double2(std::cos(a), std::sin(a));
    }
    m.resize((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) m[(size_t)j * n + k] = tw[(int)(((long long)j * k) % n)];       // the exact integer argument
}

// piq's frequency axis after ifftshift: even n: [-n/2, n/2) / n; odd n: [-(n-1)/2, (n-1)/2] / (n-1)
void freq_axis(int n, std::vector<double>& f)
{
    f.resize(n);
    for (int i = 0; i < n; ++i) {
        const int src = (i + n / 2) % n;
        f[i] = (n % 2) ? ((double)src - (double)(n - 1) / 2.0) / (double)(n - 1) : ((double)src - (double)n / 2.0) / (double)n;
    }
}

void build_filters(int h, int w, std::vector<double>& filt, NoiseConsts& nc)
{
    const size_t hw = (size_t)h * w;
    std::vector<double> fx, fy;
    freq_axis(h, fx);
    freq_axis(w, fy);
    filt.assign(NF * hw, 0.0);
    const double theta_sigma = PI / (NO * 1.2), lsf = std::log(0.55);
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const bool dc = i == 0 && j == 0;
            const double r0 = std::sqrt(fx[i] * fx[i] + fy[j] * fy[j]);
            const double theta = std::atan2(-fy[j], fx[i]), st = std::sin(theta), ct = std::cos(theta);
            const double lp = 1.0 / (1.0 + std::pow(r0 / 0.45, 30.0));
            const double r = dc ? 1.0 : r0;
            double gab[NS];
            for (int s = 0; s < NS; ++s) {
                const double omega0 = 1.0 / (6.0 * (double)(1 << s));
                const double lg = std::log(r / omega0);
                gab[s] = dc ? 0.0 : std::exp(-(lg * lg) / (2.0 * lsf * lsf)) * lp;
            }
            for (int o = 0; o < NO; ++o) {
                const double angl = o * PI / NO;
                const double ds = st * std::cos(angl) - ct * std::sin(angl), dcs = ct * std::cos(angl) + st * std::sin(angl);
                const double dth = std::fabs(std::atan2(ds, dcs));
                const double spread = std::exp(-(dth * dth) / (2.0 * theta_sigma * theta_sigma));
                for (int s = 0; s < NS; ++s) filt[(size_t)(o * NS + s) * hw + (size_t)i * w + j] = spread * gab[s];
            }
        }
    // em_n = sum filt[o, 0]^2.  With g = Re(ifft2 filt) sqrt(h w): Re(ifft2 f) = ifft2 of f's even part fe(k) = (f(k) + f(-k)) / 2, so by
    // Parseval sum_px g_s g_t = sum_k fe_s(k) fe_t(k): the two noise sums without a transform
    for (int o = 0; o < NO; ++o) {
        double em = 0.0, an2 = 0.0, aiaj = 0.0;
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) {
                const size_t at = (size_t)i * w + j, neg = (size_t)((h - i) % h) * w + (size_t)((w - j) % w);
                double fe[NS];
                for (int s = 0; s < NS; ++s) {
                    const double* f = filt.data() + (size_t)(o * NS + s) * hw;
                    fe[s] = 0.5 * (f[at] + f[neg]);
                    an2 += fe[s] * fe[s];
                }
                for (int s = 0; s < NS; ++s)
                    for (int t = s + 1; t < NS; ++t) aiaj += fe[s] * fe[t];
                const double f0 = filt[(size_t)(o * NS) * hw + at];
                em += f0 * f0;
            }
        nc.em_n[o] = em;
        nc.sum_an2[o] = an2;
        nc.sum_ai_aj[o] = aiaj;
    }
}

}   // namespace

struct xsd_fsim {
    void* ws = nullptr;
    size_t ws_bytes = 0;
    Plan plans[XSD_FSIM_PLANS];
    unsigned long long clock = 0;
    int B = 0, h = 0, w = 0;          // the last xsd_fsim_eval that was enqueued: batch and pooled size (0: none yet)
};

#define FSIM_HIPCHK(expr)                                                                                                      \
    do {                                                                                                                       \
        hipError_t _e = (expr);                                                                                                \
        if (_e != hipSuccess) return fail(XSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace {

int upload(void** dst, const void* src, size_t bytes)
{
    if (xsd::dev_alloc(dst, bytes) != hipSuccess) { *dst = nullptr; return fail(XSD_ERR_NOMEM, "xsd_fsim: plan allocation of %zu bytes failed", bytes); }
    FSIM_HIPCHK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    FSIM_HIPCHK(hipDeviceSynchronize());      // stream 0's upload is on the device before the eval's launches on a non-blocking stream read the plan
    return XSD_OK;
}

// the plan of (h, w): the cached one, or a new one in the least recently used slot
int get_plan(xsd_fsim* m, int h, int w, hipStream_t st, Plan** out)
{
    Plan* lru = &m->plans[0];
    for (Plan& p : m->plans) {
        if (p.h == h && p.w == w) { p.stamp = ++m->clock; *out = &p; return XSD_OK; }
        if (p.stamp < lru->stamp) lru = &p;
    }
    if (lru->h) {
        FSIM_HIPCHK(hipStreamSynchronize(st));        // launches that read the evicted plan are done
        free_plan(*lru);
    }
    std::vector<double2> mat;
    std::vector<double> filt;
    Plan p;
    build_filters(h, w, filt, p.nc);
    dft_matrix(h, mat);
    int rc = upload((void**)&p.Wh, mat.data(), mat.size() * sizeof(double2));
    if (rc == XSD_OK) {
        if (w == h) p.Ww = p.Wh;
        else { dft_matrix(w, mat); rc = upload((void**)&p.Ww, mat.data(), mat.size() * sizeof(double2)); }
    }
    if (rc == XSD_OK) rc = upload((void**)&p.filt, filt.data(), filt.size() * sizeof(double));
    if (rc != XSD_OK) { free_plan(p); return rc; }
    p.h = h; p.w = w; p.stamp = ++m->clock;
    *lru = p;
    *out = lru;
    return XSD_OK;
}

int reserve(xsd_fsim* m, size_t bytes, hipStream_t st, const char* who)
{
    if (bytes <= m->ws_bytes) return XSD_OK;
    FSIM_HIPCHK(hipStreamSynchronize(st));
    if (m->ws) FSIM_HIPCHK(xsd::dev_free(m->ws));
    m->ws = nullptr; m->ws_bytes = 0;
    if (xsd::dev_alloc(&m->ws, bytes) != hipSuccess) return fail(XSD_ERR_NOMEM, "%s: workspace allocation of %zu bytes failed", who, bytes);
    m->ws_bytes = bytes;
    return XSD_OK;
}

Opnd opnd(const void* p, int kind, int conj, long long ld, long long bstride, int bdiv = 1, const double* filt = nullptr, long long fstride = 0)
{
    Opnd o;
    o.p = p; o.kind = kind; o.conj = conj; o.bdiv = bdiv; o.ld = ld; o.bstride = bstride; o.filt = filt; o.fstride = fstride;
    return o;
}

void cgemm(hipStream_t st, const Opnd& A, const Opnd& B, void* C, int c_f32, double scale, int M, int N, int K, int batch)
{
    hipLaunchKernelGGL(cgemm_kernel, dim3(cdiv(N, GN), cdiv(M, GM), batch), dim3(256), 0, st, A, B, C, c_f32, scale, M, N, K);
}

// workspace layout of one (B, h, w): computed in one place, for xsd_fsim_eval and xsd_fsim_test_stage
struct FsimLayout {
    size_t hw, S2;
    int tiles_x, ntiles;
    size_t o_pool, o_y, o_f, o_z, o_eo, o_en, o_an, o_a0, o_T, o_part, bytes;
};

FsimLayout fsim_layout(int B, int h, int w)
{
    FsimLayout L;
    const size_t hw = (size_t)h * w, S2 = 2 * (size_t)B;
    L.hw = hw; L.S2 = S2;
    L.tiles_x = cdiv(w, TW); L.ntiles = L.tiles_x * cdiv(h, TH);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    L.o_pool = take(S2 * hw * sizeof(double));
    L.o_y = take(S2 * hw * sizeof(double2));
    L.o_f = take(S2 * hw * sizeof(double2));
    L.o_z = take(S2 * NF * hw * sizeof(double2));
    L.o_eo = take(S2 * NF * hw * sizeof(float2));
    L.o_en = take(S2 * NO * hw * sizeof(double));
    L.o_an = take(S2 * NO * hw * sizeof(double));
    L.o_a0 = take(S2 * NO * hw * sizeof(float));
    L.o_T = take(S2 * NO * sizeof(double));
    L.o_part = take((size_t)B * L.ntiles * 2 * sizeof(double));
    L.bytes = off;
    return L;
}

}   // namespace

int xsd_fsim_create(xsd_fsim** out)
{
    if (!out) return fail(XSD_ERR_ARG, "xsd_fsim_create: null output pointer");
    xsd_fsim* m = new (std::nothrow) xsd_fsim();
    if (!m) return fail(XSD_ERR_NOMEM, "out of host memory");
    *out = m;
    return XSD_OK;
}

void xsd_fsim_destroy(xsd_fsim* m)
{
    if (!m) return;
    for (Plan& p : m->plans) free_plan(p);
    xsd::dev_free(m->ws);
    delete m;
}

int xsd_fsim_eval(xsd_fsim* m, const float* dev_preds, const float* dev_target, double* dev_out, int B, int C, int H, int W, void* stream)
{
    if (!m || !dev_preds || !dev_target || !dev_out) return fail(XSD_ERR_ARG, "xsd_fsim_eval: null pointer");
    if (B < 1 || B > 2047) return fail(XSD_ERR_ARG, "xsd_fsim_eval: B must be 1..2047 (got %d)", B);
    if (C != 1) return fail(XSD_ERR_ARG, "xsd_fsim_eval: C must be 1 (got %d): only single-channel images (piq's chromatic / YIQ branch is not built)", C);
    if (H < 1 || W < 1) return fail(XSD_ERR_ARG, "xsd_fsim_eval: H and W must be positive (got %d x %d)", H, W);
    const int ks = std::max(1, (int)std::nearbyint((double)std::min(H, W) / 256.0));      // Python's round: ties to even
    const int h = H / ks, w = W / ks;
    if (h < 3 || w < 3 || h > MAX_SIDE || w > MAX_SIDE)
        return fail(XSD_ERR_ARG, "xsd_fsim_eval: the pooled image must be 3..%d pixels a side (got %d x %d -> %d x %d with the %d x %d mean)",
                    MAX_SIDE, H, W, h, w, ks, ks);
    hipStream_t st = (hipStream_t)stream;
    Plan* P = nullptr;
    int rc = get_plan(m, h, w, st, &P);
    if (rc != XSD_OK) return rc;

    const FsimLayout L = fsim_layout(B, h, w);
    const size_t hw = L.hw, S2 = L.S2;
    const int tiles_x = L.tiles_x, ntiles = L.ntiles;
    m->B = 0;                                      // nothing to read back until this eval is enqueued whole
    rc = reserve(m, L.bytes, st, "xsd_fsim_eval");
    if (rc != XSD_OK) return rc;
    char* ws = (char*)m->ws;
    double* pooled = (double*)(ws + L.o_pool);
    double2 *Y = (double2*)(ws + L.o_y), *F = (double2*)(ws + L.o_f), *Z = (double2*)(ws + L.o_z);
    float2* EO = (float2*)(ws + L.o_eo);
    double *EN = (double*)(ws + L.o_en), *AN = (double*)(ws + L.o_an), *T = (double*)(ws + L.o_T), *part = (double*)(ws + L.o_part);
    float* A0 = (float*)(ws + L.o_a0);

    const dim3 blk(TW, TH);
    // 1
    hipLaunchKernelGGL(pool_kernel, dim3(ntiles, (unsigned)S2), blk, 0, st, dev_preds, dev_target, pooled, B, H, W, h, w, ks, tiles_x);
    // 2: Y = P * Ww
    cgemm(st, opnd(pooled, K_RF64, 0, w, (long long)hw), opnd(P->Ww, K_CF64, 0, w, 0), Y, 0, 1.0, h, w, w, (int)S2);
    // 3: F = Wh * Y
    cgemm(st, opnd(P->Wh, K_CF64, 0, h, 0), opnd(Y, K_CF64, 0, w, (long long)hw), F, 0, 1.0, h, w, h, (int)S2);
    // 4: Z[sb * NF + f] = conj(Wh) * (F[sb] . filt[f])
    cgemm(st, opnd(P->Wh, K_CF64, 1, h, 0), opnd(F, K_CF64, 0, w, (long long)hw, NF, P->filt, (long long)hw), Z, 0, 1.0, h, w, h, (int)(S2 * NF));
    // 5: eo = Z * conj(Ww) / (h w)
    cgemm(st, opnd(Z, K_CF64, 0, w, (long long)hw), opnd(P->Ww, K_CF64, 1, w, 0), EO, 1, 1.0 / (double)hw, h, w, w, (int)(S2 * NF));
    // 6
    hipLaunchKernelGGL(pc_point_kernel, dim3(cdiv((int)hw, NT), (unsigned)S2, NO), blk, 0, st, (const float2*)EO, EN, AN, A0, (int)hw);
    // 7
    hipLaunchKernelGGL(median_T_kernel, dim3((unsigned)(S2 * NO)), dim3(MED_NT), 0, st, (const float*)A0, T, P->nc, (int)hw);
    // 8
    hipLaunchKernelGGL(fsim_map_kernel, dim3(ntiles, B), blk, 0, st, (const double*)pooled, (const double*)EN, (const double*)AN, (const double*)T,
                       part, B, h, w, tiles_x, ntiles);
    // 9
    hipLaunchKernelGGL(fsim_finish_kernel, dim3(B), blk, 0, st, (const double*)part, dev_out, ntiles);
    FSIM_HIPCHK(hipGetLastError());
    m->B = B; m->h = h; m->w = w;
    return XSD_OK;
}

int xsd_fsim_test_stage(xsd_fsim* m, int stage, void* dev_dst, int64_t dst_bytes, int* info, void* stream)
{
    if (!m || !dev_dst || !info) return fail(XSD_ERR_ARG, "xsd_fsim_test_stage: null pointer");
    if (stage < 0 || stage >= XSD_FSIM_STAGES) return fail(XSD_ERR_ARG, "xsd_fsim_test_stage: unknown stage %d (0..%d)", stage, XSD_FSIM_STAGES - 1);
    const Plan* P = nullptr;
    if (m->B)
        for (const Plan& p : m->plans)
            if (p.h == m->h && p.w == m->w) P = &p;
    if (!m->B || !m->ws || !P) return fail(XSD_ERR_ARG, "xsd_fsim_test_stage: this handle has not evaluated anything yet (or its plan is gone)");
    const FsimLayout L = fsim_layout(m->B, m->h, m->w);
    const size_t hw = L.hw, S2 = L.S2;
    size_t off = 0, bytes = 0;
    int lead = (int)S2;
    const void* src = nullptr;                                 // outside the workspace: the plan
    hipMemcpyKind kind = hipMemcpyDeviceToDevice;
    switch (stage) {
    case XSD_FSIM_STAGE_POOLED: off = L.o_pool; bytes = S2 * hw * sizeof(double); break;
    case XSD_FSIM_STAGE_EO: off = L.o_eo; bytes = S2 * NF * hw * sizeof(float2); break;
    case XSD_FSIM_STAGE_EN: off = L.o_en; bytes = S2 * NO * hw * sizeof(double); break;
    case XSD_FSIM_STAGE_AN: off = L.o_an; bytes = S2 * NO * hw * sizeof(double); break;
    case XSD_FSIM_STAGE_A0SQ: off = L.o_a0; bytes = S2 * NO * hw * sizeof(float); break;
    case XSD_FSIM_STAGE_T: off = L.o_T; bytes = S2 * NO * sizeof(double); break;
    case XSD_FSIM_STAGE_PART: off = L.o_part; bytes = (size_t)m->B * L.ntiles * 2 * sizeof(double); lead = m->B; break;
    case XSD_FSIM_STAGE_FILT: src = P->filt; bytes = (size_t)NF * hw * sizeof(double); lead = NF; break;
    default: src = &P->nc; bytes = sizeof(NoiseConsts); lead = 3; kind = hipMemcpyHostToDevice; break;
    }
    const bool part = stage == XSD_FSIM_STAGE_PART;
    info[0] = lead; info[1] = m->h; info[2] = m->w; info[3] = part ? 2 : 0;
    info[4] = part ? L.tiles_x : 0; info[5] = part ? L.ntiles : 0; info[6] = part ? TH : 0; info[7] = part ? TW : 0;
    if (dst_bytes < 0 || (size_t)dst_bytes < bytes)
        return fail(XSD_ERR_ARG, "xsd_fsim_test_stage: buffer too small for stage %d: %lld bytes given, %zu needed", stage, (long long)dst_bytes, bytes);
    if (!src) {
        if (off + bytes > m->ws_bytes) return fail(XSD_ERR_ARG, "xsd_fsim_test_stage: the region lies outside the workspace");
        src = (const char*)m->ws + off;
    }
    if (kind == hipMemcpyHostToDevice) FSIM_HIPCHK(hipMemcpy(dev_dst, src, bytes, kind));      // 96 bytes of pageable host memory
    else FSIM_HIPCHK(hipMemcpyAsync(dev_dst, src, bytes, kind, (hipStream_t)stream));
    return XSD_OK;
}

int xsd_fsim_test_dft2(xsd_fsim* m, const float* dev_in, float* dev_out, int B, int n1, int n2, int inverse, void* stream)
{
    if (!m || !dev_in || !dev_out) return fail(XSD_ERR_ARG, "xsd_fsim_test_dft2: null pointer");
    if (B < 1 || B > 65535) return fail(XSD_ERR_ARG, "xsd_fsim_test_dft2: B must be 1..65535 (got %d)", B);
    if (n1 < 3 || n2 < 3 || n1 > MAX_SIDE || n2 > MAX_SIDE)
        return fail(XSD_ERR_ARG, "xsd_fsim_test_dft2: n1 and n2 must be 3..%d (got %d x %d)", MAX_SIDE, n1, n2);
    hipStream_t st = (hipStream_t)stream;
    Plan* P = nullptr;
    int rc = get_plan(m, n1, n2, st, &P);
    if (rc != XSD_OK) return rc;
    const size_t n = (size_t)n1 * n2;
    rc = reserve(m, align256((size_t)B * n * sizeof(double2)), st, "xsd_fsim_test_dft2");
    if (rc != XSD_OK) return rc;
    m->B = 0;                                      // the transform's scratch overwrites the last eval's regions
    double2* tmp = (double2*)m->ws;
    if (!inverse) {
        cgemm(st, opnd(dev_in, K_CF32, 0, n2, (long long)n), opnd(P->Ww, K_CF64, 0, n2, 0), tmp, 0, 1.0, n1, n2, n2, B);
        cgemm(st, opnd(P->Wh, K_CF64, 0, n1, 0), opnd(tmp, K_CF64, 0, n2, (long long)n), dev_out, 1, 1.0, n1, n2, n1, B);
    } else {
        cgemm(st, opnd(P->Wh, K_CF64, 1, n1, 0), opnd(dev_in, K_CF32, 0, n2, (long long)n), tmp, 0, 1.0, n1, n2, n1, B);
        cgemm(st, opnd(tmp, K_CF64, 0, n2, (long long)n), opnd(P->Ww, K_CF64, 1, n2, 0), dev_out, 1, 1.0 / (double)n, n1, n2, n2, B);
    }
    FSIM_HIPCHK(hipGetLastError());
    return XSD_OK;
}

int xsd_fsim_test_median(const float* dev_in, float* dev_out, int rows, int n, void* stream)
{
    if (!dev_in || !dev_out) return fail(XSD_ERR_ARG, "xsd_fsim_test_median: null pointer");
    if (rows < 1 || n < 1) return fail(XSD_ERR_ARG, "xsd_fsim_test_median: rows and n must be positive (got %d, %d)", rows, n);
    hipLaunchKernelGGL(median_kernel, dim3(rows), dim3(MED_NT), 0, (hipStream_t)stream, dev_in, dev_out, n);
    FSIM_HIPCHK(hipGetLastError());
    return XSD_OK;
}
