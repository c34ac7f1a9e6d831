// restormer.hip -- the reference's Restormer denoiser (models/transformer/restormer.py:217-406), FORWARD ONLY, in exact fp32.
//
// Every product is an fp32 FMA on the vector ALUs (xsd_set_math does not apply: this path has no split modes); the long reductions
// are carried in double: the LayerNorm statistics, and the channel attention's row norms and C_h x C_h Gram over all pixels of an
// image (fp32 chains of 64 pixels, summed per fixed pixel range in double, the ranges combined in a fixed order in double).  No float atomics anywhere: an image's output is bitwise independent
// of the batch it shares and of the run.
//
// Tensors are NCHW fp32 with a batch stride per view, so that torch.cat([up, skip], 1) of the decoder (restormer.py:383-396) is a
// channel PREFIX of one slab: the encoder level writes its output into the slab's upper channels, the Upsample conv into the
// lower ones, and reduce_chan reads the slab as one tensor.  PixelUnshuffle / PixelShuffle (:185-214) are the store addressing
// of the 3x3 conv in front of them.
//
// Kernels (DESIGN.md "Restormer" has the per-kernel byte / FLOP roof):
//   rst_pw_kernel      1x1 conv, optionally with the channel LayerNorm (:25-73) of its input fused in front, per-image or shared
//                      weights ([cin][cout], packed), bias, residual add (in place).  Serves qkv (:124), project_in (:110), the
//                      attention output (attn @ v folded into project_out, below), the FFN project_out (+ residual) and
//                      reduce_chan_level3 / 2 (:320-353).
//   rst_dw_kernel      depthwise 3x3, zero pad 1, bias; in gate mode the FFN's gelu(x1) * x2 (:96-104) over the two halves.
//   rst_gram_kernel    per image, head and pixel range: the raw Gram q k^T and the squared row norms of q and k (fp32 FMA chains
//                      over 64-pixel rounds, the rounds summed in double).
//   rst_attn_kernel    per image and head: combine the ranges (double, fixed order), F.normalize (eps 1e-12) as a division of the
//                      Gram by the two norms, x temperature, softmax over the last dim, then fold project_out into it:
//                      project_out(attn @ v) = (W_po blockdiag(attn_h)) v, i.e. a per-image C x C 1x1 conv applied to v.
//   rst_wgram_kernel, rst_wsoftmax_kernel, rst_wfold_kernel
//                      the same channel attention from 65 to 128 channels per head (the published dim 48 runs 96 on one head at
//                      decoder level 1): the Gram tiled over the grid, the softmax and the fold as kernels of their own; the
//                      arithmetic of the two kernels above entry by entry.
//   rst_conv3_kernel   dense 3x3 conv (patch_embed :160, Downsample / Upsample bodies, output :366; summed in double) with plain,
//                      PixelUnshuffle(2) or PixelShuffle(2) store and the `+ inp_img` skip (:404).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/xsd.h"

#include "xsd_err.h"
#include "xsd_mem.h"
#define rfail xsd::failf      // the thread-local message of xsd_last_error()

namespace {

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
constexpr int PW_PX = 64;     // pixels per workgroup: lane = pixel
constexpr int PW_CO = 64;     // output channels per workgroup: 16 per wave
constexpr int PW_CI = 32;     // input channels per LDS round

struct PwP {
    const float* x; long long xbs; int cin;
    const float* lnw; const float* lnb; int ln;   // ln: 0 none, 1 WithBias, 2 BiasFree (lnb unused)
    const float* w; long long wbs;                // [cin][cout]; wbs: per-image stride (0: shared)
    const float* bias;                            // [cout] or null
    const float* res; long long resbs;            // v += res (may alias y: same element, same thread) or null
    float* y; long long ybs; int cout;
    long long HW;
};

__global__ __launch_bounds__(256) void rst_pw_kernel(const PwP P)
{
    __shared__ __attribute__((aligned(16))) float xs[PW_CI][PW_PX];
    __shared__ __attribute__((aligned(16))) float wsm[PW_CI][PW_CO];
    __shared__ double red[4][PW_PX], mu_s[PW_PX];
    __shared__ float mu_f[PW_PX], sd_s[PW_PX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p0 = (long long)blockIdx.x * PW_PX;
    const int co0 = blockIdx.y * PW_CO, b = blockIdx.z;
    const long long p = p0 + lane;
    const bool pin = p < P.HW;
    const float* xb = P.x + (long long)b * P.xbs;
    if (P.ln) {
        // mean and biased variance over the channels of each pixel, two passes (x.mean / x.var(unbiased=False)), summed in double
        double s = 0.0;
        if (pin)
            for (int c = wave; c < P.cin; c += 4) s += (double)xb[(long long)c * P.HW + p];
        red[wave][lane] = s;
        __syncthreads();
        if (wave == 0) mu_s[lane] = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / P.cin;
        __syncthreads();
        const double mu = mu_s[lane];
        double q = 0.0;
        if (pin)
            for (int c = wave; c < P.cin; c += 4) {
                const double d = (double)xb[(long long)c * P.HW + p] - mu;
                q = fma(d, d, q);
            }
        red[wave][lane] = q;
        __syncthreads();
        if (wave == 0) {
            mu_f[lane] = (float)mu_s[lane];
            sd_s[lane] = (float)sqrt((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / P.cin + 1e-5);
        }
    }
    const float* wb = P.w + (long long)b * P.wbs;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    for (int ci0 = 0; ci0 < P.cin; ci0 += PW_CI) {
        __syncthreads();
        for (int i = tid; i < PW_CI * PW_PX; i += 256) {
            const int c = i >> 6, px = i & 63, ci = ci0 + c;
            const long long pp = p0 + px;
            float v = 0.f;
            if (ci < P.cin && pp < P.HW) {
                v = xb[(long long)ci * P.HW + pp];
                if (P.ln == 1) v = (v - mu_f[px]) / sd_s[px] * P.lnw[ci] + P.lnb[ci];
                else if (P.ln == 2) v = v / sd_s[px] * P.lnw[ci];
            }
            xs[c][px] = v;
        }
        for (int i = tid; i < PW_CI * PW_CO; i += 256) {
            const int c = i / PW_CO, col = i % PW_CO, ci = ci0 + c, co = co0 + col;
            wsm[c][col] = (ci < P.cin && co < P.cout) ? wb[(long long)ci * P.cout + co] : 0.f;
        }
        __syncthreads();
        const int nc = min(PW_CI, P.cin - ci0);
        for (int c = 0; c < nc; ++c) {
            const float xv = xs[c][lane];
            const float4* wr = reinterpret_cast<const float4*>(&wsm[c][wave * 16]);
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const float4 w4 = wr[k4];
                acc[4 * k4 + 0] = fmaf(w4.x, xv, acc[4 * k4 + 0]);
                acc[4 * k4 + 1] = fmaf(w4.y, xv, acc[4 * k4 + 1]);
                acc[4 * k4 + 2] = fmaf(w4.z, xv, acc[4 * k4 + 2]);
                acc[4 * k4 + 3] = fmaf(w4.w, xv, acc[4 * k4 + 3]);
            }
        }
    }
    if (!pin) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int co = co0 + wave * 16 + k;
        if (co >= P.cout) break;
        float v = acc[k] + (P.bias ? P.bias[co] : 0.f);
        if (P.res) v += P.res[(long long)b * P.resbs + (long long)co * P.HW + p];
        P.y[(long long)b * P.ybs + (long long)co * P.HW + p] = v;
    }
}

struct DwP {
    const float* x; long long xbs;
    const float* w; const float* bias;    // [channels][9], [channels] or null
    float* y; long long ybs;
    int cout;                             // output channels (gate: the hidden width; input channels = 2 cout)
    int gate;
    int H, W;
};

__device__ __forceinline__ float dw9(const float* xc, const float* wc, int gy, int gx, int H, int W)
{
    float acc = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = gy + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = gx + dx;
            if (xx < 0 || xx >= W) continue;
            acc = fmaf(wc[(dy + 1) * 3 + dx + 1], xc[(long long)yy * W + xx], acc);
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void rst_dw_kernel(const DwP P)
{
    const long long HW = (long long)P.H * P.W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const int gy = (int)(p / P.W), gx = (int)(p - (long long)gy * P.W);
    const float* xb = P.x + (long long)b * P.xbs;
    float v = dw9(xb + (long long)c * HW, P.w + c * 9, gy, gx, P.H, P.W) + (P.bias ? P.bias[c] : 0.f);
    if (P.gate) {
        const int c2 = c + P.cout;
        const float v2 = dw9(xb + (long long)c2 * HW, P.w + c2 * 9, gy, gx, P.H, P.W) + (P.bias ? P.bias[c2] : 0.f);
        v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f)) * v2;        // F.gelu (exact erf form) * x2
    }
    P.y[(long long)b * P.ybs + (long long)c * HW + p] = v;
}

constexpr int AT_MAXCH = 64;                                          // channels per head (rst_gram_kernel / rst_attn_kernel)
constexpr int AT_PX = 64;                                             // pixels per LDS round
constexpr int AT_MAXE = (AT_MAXCH * AT_MAXCH + 2 * AT_MAXCH + 255) / 256;   // entries per thread

struct GramP {
    const float* qkv; long long bs;      // [B][3C][HW]: q = channels [0, C), k = [C, 2C)
    int C, ch;
    long long HW;
    int chunk, nsplit;                   // pixels per range, ranges per image
    double* part;                        // [B][heads][nsplit][ch*ch + 2ch]
};

__global__ __launch_bounds__(256) void rst_gram_kernel(const GramP P)
{
    __shared__ float qs[AT_MAXCH][AT_PX + 1], ks[AT_MAXCH][AT_PX + 1];
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y, ch = P.ch, tid = threadIdx.x;
    const int E = ch * ch + 2 * ch;
    const float* qb = P.qkv + (long long)b * P.bs + (long long)h * ch * P.HW;
    const float* kb = qb + (long long)P.C * P.HW;
    const long long pb = (long long)s * P.chunk, pe = min(P.HW, pb + P.chunk);
    double acc[AT_MAXE];          // fp32 FMA chain over one 64-pixel round, rounds summed in double
#pragma unroll
    for (int j = 0; j < AT_MAXE; ++j) acc[j] = 0.0;
    for (long long r0 = pb; r0 < pe; r0 += AT_PX) {
        __syncthreads();
        for (int i = tid; i < ch * AT_PX; i += 256) {
            const int c = i / AT_PX, px = i % AT_PX;
            const long long pp = r0 + px;
            const bool ok = pp < pe;
            qs[c][px] = ok ? qb[(long long)c * P.HW + pp] : 0.f;
            ks[c][px] = ok ? kb[(long long)c * P.HW + pp] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < AT_MAXE; ++j) {
            const int e = tid + 256 * j;
            if (e >= E) break;
            const float *a, *c;
            if (e < ch * ch) { a = qs[e / ch]; c = ks[e % ch]; }
            else if (e < ch * ch + ch) { a = c = qs[e - ch * ch]; }
            else { a = c = ks[e - ch * ch - ch]; }
            float t = 0.f;
            for (int px = 0; px < AT_PX; ++px) t = fmaf(a[px], c[px], t);
            acc[j] += (double)t;
        }
    }
    double* out = P.part + (((long long)b * heads + h) * P.nsplit + s) * E;
#pragma unroll
    for (int j = 0; j < AT_MAXE; ++j) {
        const int e = tid + 256 * j;
        if (e < E) out[e] = acc[j];
    }
}

struct AttnP {
    const double* part; int nsplit;
    const float* temp;                   // [heads]
    const float* wpo_t;                  // project_out weight, packed [C][C] = [ci][co]
    float* mt; int C, ch;                // per-image folded matrix, [B][C][C] = [ci][co] (the layout rst_pw_kernel reads)
};

__global__ __launch_bounds__(256) void rst_attn_kernel(const AttnP P)
{
    __shared__ double g[AT_MAXCH * AT_MAXCH + 2 * AT_MAXCH];
    __shared__ float A[AT_MAXCH][AT_MAXCH + 1];
    const int h = blockIdx.x, b = blockIdx.y, heads = gridDim.x, ch = P.ch, C = P.C, tid = threadIdx.x;
    const int E = ch * ch + 2 * ch;
    const double* pb = P.part + ((long long)b * heads + h) * P.nsplit * E;
    for (int e = tid; e < E; e += 256) {
        double s = 0.0;
        for (int k = 0; k < P.nsplit; ++k) s += pb[(long long)k * E + e];
        g[e] = s;
    }
    __syncthreads();
    if (tid < ch) {
        const int i = tid;
        const double nq = fmax(sqrt(g[ch * ch + i]), 1e-12), t = (double)P.temp[h];
        double mx = -INFINITY;
        for (int j = 0; j < ch; ++j) {
            const double nk = fmax(sqrt(g[ch * ch + ch + j]), 1e-12);
            const double l = g[i * ch + j] / (nq * nk) * t;
            g[i * ch + j] = l;
            mx = fmax(mx, l);
        }
        double den = 0.0;
        for (int j = 0; j < ch; ++j) den += exp(g[i * ch + j] - mx);
        for (int j = 0; j < ch; ++j) A[i][j] = (float)(exp(g[i * ch + j] - mx) / den);
    }
    __syncthreads();
    // M[co][h ch + j] = sum_i W_po[co][h ch + i] A[i][j], stored transposed: mt[b][h ch + j][co]
    float* mb = P.mt + (long long)b * C * C;
    for (int e = tid; e < ch * C; e += 256) {
        const int j = e / C, co = e % C;
        double s = 0.0;
        for (int i = 0; i < ch; ++i) s = fma((double)P.wpo_t[(long long)(h * ch + i) * C + co], (double)A[i][j], s);
        mb[(long long)(h * ch + j) * C + co] = (float)s;
    }
}

// ---- the wide path: 65 to 128 channels per head (the kernels take any ch in [1, 128]) -----------------------------------------------
// The same arithmetic, entry by entry, as the two kernels above (on a width both take, the outputs are bitwise equal), with the Gram
// tiled over the grid instead of held whole by one workgroup: a workgroup owns a 64 x 64 tile of q k^T over one pixel range, a thread a
// 4 x 4 block of it in registers.  The softmax and the fold are kernels of their own, attn in an fp32 scratch between them.
constexpr int WD_MAXCH = 128;                                         // channels per head
constexpr int WD_T = 64;                                              // Gram tile: 64 q rows x 64 k rows
constexpr int WD_LD = AT_PX + 4;                                      // LDS row stride: float4 reads, 16 rows on 16 different 16-B slots
constexpr int WS_ROWS = 8;                                            // attn rows per softmax workgroup

__global__ __launch_bounds__(256) void rst_wgram_kernel(const GramP P)
{
    __shared__ __attribute__((aligned(16))) float qs[WD_T][WD_LD], ks[WD_T][WD_LD];
    const int ch = P.ch, tid = threadIdx.x, nt = (ch + WD_T - 1) / WD_T, heads = gridDim.y / (nt * nt);
    const int s = blockIdx.x, h = blockIdx.y / (nt * nt), tile = blockIdx.y % (nt * nt), b = blockIdx.z;
    const int i0 = (tile / nt) * WD_T, j0 = (tile % nt) * WD_T;       // first q row / k row of the tile
    const int ni = min(WD_T, ch - i0), nj = min(WD_T, ch - j0);       // rows of it inside the head
    const int nr = (ni + 15) / 16, ns = (nj + 15) / 16;               // 16-row groups with a row inside (the same for every thread)
    const int ti = tid >> 4, tj = tid & 15;                           // the thread's entries: q rows ti + 16 r, k rows tj + 16 s
    const int E = ch * ch + 2 * ch;
    const float* qb = P.qkv + (long long)b * P.bs + (long long)h * ch * P.HW;
    const float* kb = qb + (long long)P.C * P.HW;
    const long long pb = (long long)s * P.chunk, pe = min(P.HW, pb + P.chunk);
    // the tiles of the first tile column carry the q norms of their rows, those of the first tile row the k norms: waves 0 and 1
    const float* nrow = nullptr;
    if (tile % nt == 0 && tid < ni) nrow = qs[tid];
    else if (tile / nt == 0 && tid >= 64 && tid - 64 < nj) nrow = ks[tid - 64];
    double acc[4][4], nacc = 0.0;      // fp32 FMA chain over one 64-pixel round, rounds summed in double
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (long long r0 = pb; r0 < pe; r0 += AT_PX) {
        __syncthreads();
        for (int i = tid; i < WD_T * AT_PX; i += 256) {
            const int c = i / AT_PX, px = i % AT_PX;
            const long long pp = r0 + px;
            const bool ok = pp < pe;
            qs[c][px] = (ok && c < ni) ? qb[(long long)(i0 + c) * P.HW + pp] : 0.f;
            ks[c][px] = (ok && c < nj) ? kb[(long long)(j0 + c) * P.HW + pp] : 0.f;
        }
        __syncthreads();
        float t[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) t[r][c] = 0.f;
        for (int px = 0; px < AT_PX; px += 4) {
            float4 kv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < ns) kv[c] = *reinterpret_cast<const float4*>(&ks[tj + 16 * c][px]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r >= nr) break;
                const float4 qv = *reinterpret_cast<const float4*>(&qs[ti + 16 * r][px]);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c >= ns) break;
                    float v = t[r][c];
                    v = fmaf(qv.x, kv[c].x, v);
                    v = fmaf(qv.y, kv[c].y, v);
                    v = fmaf(qv.z, kv[c].z, v);
                    v = fmaf(qv.w, kv[c].w, v);
                    t[r][c] = v;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] += (double)t[r][c];
        if (nrow) {
            float v = 0.f;
            for (int px = 0; px < AT_PX; px += 4) {
                const float4 a = *reinterpret_cast<const float4*>(&nrow[px]);
                v = fmaf(a.x, a.x, v);
                v = fmaf(a.y, a.y, v);
                v = fmaf(a.z, a.z, v);
                v = fmaf(a.w, a.w, v);
            }
            nacc += (double)v;
        }
    }
    double* out = P.part + (((long long)b * heads + h) * P.nsplit + s) * E;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = ti + 16 * r, j = tj + 16 * c;
            if (i < ni && j < nj) out[(i0 + i) * ch + j0 + j] = acc[r][c];
        }
    if (nrow) out[ch * ch + (tid < 64 ? i0 + tid : ch + j0 + tid - 64)] = nacc;
}

struct WSoftP {
    const double* part; int nsplit;
    const float* temp;                   // [heads]
    float* attn; int ch;                 // [B][heads][ch][ch]
};

// WS_ROWS rows of one head's attn: the ranges combined (double, ascending), the Gram divided by the two clamped norms, x temperature, the
// softmax of each row.  The logits and the exponentials are computed entry by entry in parallel; the running maximum and the
// denominator of a row are taken by one thread over ascending j, as rst_attn_kernel takes them.
__global__ __launch_bounds__(256) void rst_wsoftmax_kernel(const WSoftP P)
{
    __shared__ double l[WS_ROWS][WD_MAXCH], nk[WD_MAXCH], nq[WS_ROWS], mx_s[WS_ROWS], den_s[WS_ROWS];
    const int i0 = blockIdx.x * WS_ROWS, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y, ch = P.ch, tid = threadIdx.x;
    const int rows = min(WS_ROWS, ch - i0), E = ch * ch + 2 * ch;
    const double* pb = P.part + ((long long)b * heads + h) * P.nsplit * E;
    for (int e = tid; e < rows * ch + ch + rows; e += 256) {
        const int r = e / ch, j = e % ch;                  // r == rows: the k norms; past them: the q norms of the rows
        const int src = e < rows * ch ? (i0 + r) * ch + j : e < rows * ch + ch ? ch * ch + ch + j : ch * ch + i0 + (e - rows * ch - ch);
        double s = 0.0;
        for (int k = 0; k < P.nsplit; ++k) s += pb[(long long)k * E + src];
        if (e < rows * ch) l[r][j] = s;
        else if (e < rows * ch + ch) nk[j] = fmax(sqrt(s), 1e-12);
        else nq[e - rows * ch - ch] = fmax(sqrt(s), 1e-12);
    }
    __syncthreads();
    const double t = (double)P.temp[h];
    for (int e = tid; e < rows * ch; e += 256) {
        const int r = e / ch, j = e % ch;
        l[r][j] = l[r][j] / (nq[r] * nk[j]) * t;
    }
    __syncthreads();
    if (tid < rows) {
        double mx = -INFINITY;
        for (int j = 0; j < ch; ++j) mx = fmax(mx, l[tid][j]);
        mx_s[tid] = mx;
    }
    __syncthreads();
    for (int e = tid; e < rows * ch; e += 256) {
        const int r = e / ch, j = e % ch;
        l[r][j] = exp(l[r][j] - mx_s[r]);
    }
    __syncthreads();
    if (tid < rows) {
        double den = 0.0;
        for (int j = 0; j < ch; ++j) den += l[tid][j];
        den_s[tid] = den;
    }
    __syncthreads();
    float* ab = P.attn + (((long long)b * heads + h) * ch + i0) * ch;
    for (int e = tid; e < rows * ch; e += 256) {
        const int r = e / ch, j = e % ch;
        ab[r * ch + j] = (float)(l[r][j] / den_s[r]);
    }
}

struct WFoldP {
    const float* attn;                   // [B][heads][ch][ch]
    const float* wpo_t;                  // project_out weight, packed [C][C] = [ci][co]
    float* mt; int C, ch;                // per-image folded matrix, [B][C][C] = [ci][co]
};

// M[co][h ch + j] = sum_i W_po[co][h ch + i] attn[i][j] (double fma over ascending i), stored transposed: mt[b][h ch + j][co]
__global__ __launch_bounds__(256) void rst_wfold_kernel(const WFoldP P)
{
    const int h = blockIdx.y, b = blockIdx.z, heads = gridDim.y, ch = P.ch, C = P.C;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ch * C) return;
    const int j = e / C, co = e % C;
    const float* ab = P.attn + ((long long)b * heads + h) * ch * ch;
    double s = 0.0;
    for (int i = 0; i < ch; ++i) s = fma((double)P.wpo_t[(long long)(h * ch + i) * C + co], (double)ab[i * ch + j], s);
    P.mt[(long long)b * C * C + (long long)(h * ch + j) * C + co] = (float)s;
}

constexpr int C3T = 16;              // 16 x 16 pixel tile per workgroup
constexpr int C3CO = 8, C3CI = 8;    // output channels per thread / input channels per LDS round

struct C3P {
    const float* x; long long xbs; int cin;
    const float* w; const float* bias;   // OIHW [cout][cin][3][3], [cout] or null
    float* y; long long ybs; int cout;
    int H, W;                            // input (= conv output) size
    int mode;                            // 0 plain, 1 PixelUnshuffle(2), 2 PixelShuffle(2)
    const float* skip; long long skipbs; // plain mode: v += skip[co] (the `+ inp_img` of the output conv)
};

__global__ __launch_bounds__(256) void rst_conv3_kernel(const C3P P)
{
    __shared__ float xin[C3CI][C3T + 2][C3T + 2];
    __shared__ double wl[C3CO][C3CI][9];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int tilesX = (P.W + C3T - 1) / C3T;
    const int x0 = ((int)blockIdx.x % tilesX) * C3T, y0 = ((int)blockIdx.x / tilesX) * C3T;
    const int co0 = blockIdx.y * C3CO, b = blockIdx.z;
    const long long HW = (long long)P.H * P.W;
    const float* xb = P.x + (long long)b * P.xbs;
    // the 9 cin products of an output are summed in double: in fp32 the chain's roundings alone put the result at 2-4x the error of a
    // correctly rounded conv, which is what the fp32 yardstick delivers at these sizes
    double acc[C3CO];
#pragma unroll
    for (int k = 0; k < C3CO; ++k) acc[k] = 0.0;
    for (int ci0 = 0; ci0 < P.cin; ci0 += C3CI) {
        __syncthreads();
        for (int i = threadIdx.x; i < C3CI * (C3T + 2) * (C3T + 2); i += 256) {
            const int c = i / ((C3T + 2) * (C3T + 2)), r = i % ((C3T + 2) * (C3T + 2));
            const int hy = r / (C3T + 2), hx = r % (C3T + 2);
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx, ci = ci0 + c;
            const bool ok = ci < P.cin && gy >= 0 && gy < P.H && gx >= 0 && gx < P.W;
            xin[c][hy][hx] = ok ? xb[(long long)ci * HW + (long long)gy * P.W + gx] : 0.f;
        }
        for (int i = threadIdx.x; i < C3CO * C3CI * 9; i += 256) {
            const int k = i / (C3CI * 9), r = i % (C3CI * 9), c = r / 9, t = r % 9;
            const int co = co0 + k, ci = ci0 + c;
            wl[k][c][t] = (co < P.cout && ci < P.cin) ? (double)P.w[((long long)co * P.cin + ci) * 9 + t] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C3CI; ++c) {
            double v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) v[t] = (double)xin[c][ty + t / 3][tx + t % 3];
#pragma unroll
            for (int k = 0; k < C3CO; ++k)
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[k] = fma(wl[k][c][t], v[t], acc[k]);
        }
    }
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx >= P.W || gy >= P.H) return;
#pragma unroll
    for (int k = 0; k < C3CO; ++k) {
        const int co = co0 + k;
        if (co >= P.cout) break;
        float v = (float)(acc[k] + (P.bias ? (double)P.bias[co] : 0.0));
        long long o;
        if (P.mode == 1) o = (long long)(co * 4 + (gy & 1) * 2 + (gx & 1)) * (HW / 4) + (long long)(gy >> 1) * (P.W / 2) + (gx >> 1);
        else if (P.mode == 2) o = (long long)(co >> 2) * 4 * HW + (long long)(2 * gy + ((co >> 1) & 1)) * (2 * P.W) + 2 * gx + (co & 1);
        else {
            o = (long long)co * HW + (long long)gy * P.W + gx;
            if (P.skip) v += P.skip[(long long)b * P.skipbs + o];
        }
        P.y[(long long)b * P.ybs + o] = v;
    }
}

// [rows][cols] -> [cols][rows] (1x1 conv weights [cout][cin] -> the [cin][cout] rst_pw_kernel reads)
__global__ __launch_bounds__(256) void rst_transpose_kernel(const float* src, float* dst, int rows, int cols)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)rows * cols) return;
    const int c = (int)(i / rows), r = (int)(i % rows);
    dst[i] = src[(long long)r * cols + c];
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct Pw1 { long long w = -1, b = -1, t = -1; int cout = 0, cin = 0; };   // flat offsets of weight / bias, offset of the packed copy

struct Blk {
    int C, heads, ch, hid;
    long long n1w, n1b, temp, qkv_dw, qkv_dwb, n2w, n2b, ffn_dw, ffn_dwb;
    Pw1 qkv, po, pin, pout;
};

} // namespace

struct xsd_restormer {
    xsd_restormer_config cfg;
    long long nparams = 0, wt_floats = 0;
    int dim = 0;
    std::vector<Blk> enc1, enc2, enc3, lat, dec3, dec2, dec1, refine;
    long long patch = 0, down12 = 0, down23 = 0, down34 = 0, up43 = 0, up32 = 0, up21 = 0, outw = 0, outb = -1;
    Pw1 red3, red2;
    std::vector<Pw1*> pw1s;
    float* wt = nullptr;
    const float* params = nullptr;
    bool packed = false;
    int B = 0, H = 0, W = 0;
    char* ws = nullptr;
    size_t ws_bytes = 0;
    float *slab1 = nullptr, *slab2 = nullptr, *dec2b = nullptr, *slab3 = nullptr, *dec3b = nullptr, *latb = nullptr;
    float *Ta = nullptr, *Tb = nullptr, *part = nullptr, *mt = nullptr, *attn = nullptr;

    ~xsd_restormer()
    {
        if (wt) xsd::dev_free(wt);
        if (ws) xsd::dev_free(ws);
    }
};

namespace {

int hidden_of(const xsd_restormer_config& c, int C) { return (int)((double)C * c.ffn_expansion_factor); }   // int(dim * f) (:82)

long long add(long long& off, long long n) { const long long o = off; off += n; return o; }

// the reference's registration order (restormer.py:142-153, :79-93, :109-121, :50-57)
void layout_blocks(xsd_restormer* r, std::vector<Blk>& v, int n, int C, int heads, long long& off)
{
    const auto& c = r->cfg;
    for (int i = 0; i < n; ++i) {
        Blk k{};
        k.C = C; k.heads = heads; k.ch = C / heads; k.hid = hidden_of(c, C);
        k.n1w = add(off, C); k.n1b = c.layernorm_bias_free ? -1 : add(off, C);
        k.temp = add(off, heads);
        k.qkv.cout = 3 * C; k.qkv.cin = C; k.qkv.w = add(off, 3ll * C * C); k.qkv.b = c.bias ? add(off, 3 * C) : -1;
        k.qkv_dw = add(off, 3ll * C * 9); k.qkv_dwb = c.bias ? add(off, 3 * C) : -1;
        k.po.cout = C; k.po.cin = C; k.po.w = add(off, 1ll * C * C); k.po.b = c.bias ? add(off, C) : -1;
        k.n2w = add(off, C); k.n2b = c.layernorm_bias_free ? -1 : add(off, C);
        k.pin.cout = 2 * k.hid; k.pin.cin = C; k.pin.w = add(off, 2ll * k.hid * C); k.pin.b = c.bias ? add(off, 2 * k.hid) : -1;
        k.ffn_dw = add(off, 2ll * k.hid * 9); k.ffn_dwb = c.bias ? add(off, 2 * k.hid) : -1;
        k.pout.cout = C; k.pout.cin = k.hid; k.pout.w = add(off, 1ll * C * k.hid); k.pout.b = c.bias ? add(off, C) : -1;
        v.push_back(k);
    }
}

void layout(xsd_restormer* r)
{
    const auto& c = r->cfg;
    const int d = c.dim;
    long long off = 0;
    r->patch = add(off, 1ll * d * c.inp_channels * 9);                                        // patch_embed.proj (bias=False)
    layout_blocks(r, r->enc1, c.num_blocks[0], d, c.heads[0], off);
    r->down12 = add(off, 1ll * (d / 2) * d * 9);
    layout_blocks(r, r->enc2, c.num_blocks[1], 2 * d, c.heads[1], off);
    r->down23 = add(off, 1ll * d * 2 * d * 9);
    layout_blocks(r, r->enc3, c.num_blocks[2], 4 * d, c.heads[2], off);
    r->down34 = add(off, 1ll * 2 * d * 4 * d * 9);
    layout_blocks(r, r->lat, c.num_blocks[3], 8 * d, c.heads[3], off);
    r->up43 = add(off, 1ll * 16 * d * 8 * d * 9);
    r->red3.cout = 4 * d; r->red3.cin = 8 * d; r->red3.w = add(off, 32ll * d * d); r->red3.b = c.bias ? add(off, 4 * d) : -1;
    layout_blocks(r, r->dec3, c.num_blocks[2], 4 * d, c.heads[2], off);
    r->up32 = add(off, 1ll * 8 * d * 4 * d * 9);
    r->red2.cout = 2 * d; r->red2.cin = 4 * d; r->red2.w = add(off, 8ll * d * d); r->red2.b = c.bias ? add(off, 2 * d) : -1;
    layout_blocks(r, r->dec2, c.num_blocks[1], 2 * d, c.heads[1], off);
    r->up21 = add(off, 1ll * 4 * d * 2 * d * 9);
    layout_blocks(r, r->dec1, c.num_blocks[0], 2 * d, c.heads[0], off);
    layout_blocks(r, r->refine, c.num_refinement_blocks, 2 * d, c.heads[0], off);
    r->outw = add(off, 1ll * c.out_channels * 2 * d * 9);
    r->outb = c.bias ? add(off, c.out_channels) : -1;
    r->nparams = off;
    long long t = 0;
    for (auto* v : {&r->enc1, &r->enc2, &r->enc3, &r->lat, &r->dec3, &r->dec2, &r->dec1, &r->refine})
        for (auto& k : *v)
            for (Pw1* p : {&k.qkv, &k.po, &k.pin, &k.pout}) r->pw1s.push_back(p);
    r->pw1s.push_back(&r->red3);
    r->pw1s.push_back(&r->red2);
    for (Pw1* p : r->pw1s) p->t = add(t, 1ll * p->cout * p->cin);
    r->wt_floats = t;
}

int nsplit_of(long long HW, int chunk) { return (int)((HW + chunk - 1) / chunk); }
constexpr int GRAM_CHUNK = 1024;       // pixels per Gram partial: a function of the image size only, never of the batch

const float* P(const xsd_restormer* r, long long off) { return off < 0 ? nullptr : r->params + off; }

hipError_t pw(hipStream_t s, const float* x, long long xbs, int cin, const float* lnw, const float* lnb, int ln, const float* w, long long wbs,
              const float* bias, const float* res, long long resbs, float* y, long long ybs, int cout, long long HW, int B)
{
    PwP p{x, xbs, cin, lnw, lnb, ln, w, wbs, bias, res, resbs, y, ybs, cout, HW};
    dim3 grid((unsigned)((HW + PW_PX - 1) / PW_PX), (unsigned)((cout + PW_CO - 1) / PW_CO), (unsigned)B);
    hipLaunchKernelGGL(rst_pw_kernel, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t conv3(hipStream_t s, const float* x, long long xbs, int cin, const float* w, const float* bias, float* y, long long ybs, int cout,
                 int H, int W, int mode, const float* skip, long long skipbs, int B)
{
    C3P p{x, xbs, cin, w, bias, y, ybs, cout, H, W, mode, skip, skipbs};
    dim3 grid((unsigned)(((W + C3T - 1) / C3T) * ((H + C3T - 1) / C3T)), (unsigned)((cout + C3CO - 1) / C3CO), (unsigned)B);
    hipLaunchKernelGGL(rst_conv3_kernel, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t dw(hipStream_t s, const float* x, long long xbs, const float* w, const float* bias, float* y, long long ybs, int cout, int gate, int H,
              int W, int B)
{
    DwP p{x, xbs, w, bias, y, ybs, cout, gate, H, W};
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(rst_dw_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)cout, (unsigned)B), dim3(256), 0, s, p);
    return hipGetLastError();
}

// the same through the wide kernels (any ch in [1, 128]): the Gram tiled over pixel range x Gram tile x head x image, attn [B][heads][ch][ch]
// in `attn` between the softmax and the fold
hipError_t attention_wide(hipStream_t s, const float* qkv, long long qbs, const float* temp, const float* wpo_t, const float* bpo, double* part,
                          float* attn, float* mt, float* X, long long xbs, int C, int heads, long long HW, int B)
{
    const int nsplit = nsplit_of(HW, GRAM_CHUNK), ch = C / heads, nt = (ch + WD_T - 1) / WD_T;
    hipError_t e;
    GramP p{qkv, qbs, C, ch, HW, GRAM_CHUNK, nsplit, part};
    hipLaunchKernelGGL(rst_wgram_kernel, dim3((unsigned)nsplit, (unsigned)(heads * nt * nt), (unsigned)B), dim3(256), 0, s, p);
    if ((e = hipGetLastError())) return e;
    WSoftP a{part, nsplit, temp, attn, ch};
    hipLaunchKernelGGL(rst_wsoftmax_kernel, dim3((unsigned)((ch + WS_ROWS - 1) / WS_ROWS), (unsigned)heads, (unsigned)B), dim3(256), 0, s, a);
    if ((e = hipGetLastError())) return e;
    WFoldP f{attn, wpo_t, mt, C, ch};
    hipLaunchKernelGGL(rst_wfold_kernel, dim3((unsigned)((ch * C + 255) / 256), (unsigned)heads, (unsigned)B), dim3(256), 0, s, f);
    if ((e = hipGetLastError())) return e;
    return pw(s, qkv + 2 * C * HW, qbs, C, nullptr, nullptr, 0, mt, (long long)C * C, bpo, X, xbs, X, xbs, C, HW, B);
}

// x += project_out(softmax(normalize(q) normalize(k)^T temperature) v) (:126-139): qkv [B][3C][HW] with a batch stride of qbs, the Gram
// partials into `part`, the per-image folded matrix into `mt`, then v through it as a per-image 1x1 conv onto X in place.  Past 64
// channels per head the wide kernels do it (`attn` is their scratch, unused below that)
hipError_t attention(hipStream_t s, const float* qkv, long long qbs, const float* temp, const float* wpo_t, const float* bpo, double* part,
                     float* attn, float* mt, float* X, long long xbs, int C, int heads, long long HW, int B)
{
    const int nsplit = nsplit_of(HW, GRAM_CHUNK), ch = C / heads;
    if (ch > AT_MAXCH) return attention_wide(s, qkv, qbs, temp, wpo_t, bpo, part, attn, mt, X, xbs, C, heads, HW, B);
    hipError_t e;
    GramP p{qkv, qbs, C, ch, HW, GRAM_CHUNK, nsplit, part};
    hipLaunchKernelGGL(rst_gram_kernel, dim3((unsigned)nsplit, (unsigned)heads, (unsigned)B), dim3(256), 0, s, p);
    if ((e = hipGetLastError())) return e;
    AttnP a{part, nsplit, temp, wpo_t, mt, C, ch};
    hipLaunchKernelGGL(rst_attn_kernel, dim3((unsigned)heads, (unsigned)B), dim3(256), 0, s, a);
    if ((e = hipGetLastError())) return e;
    return pw(s, qkv + 2 * C * HW, qbs, C, nullptr, nullptr, 0, mt, (long long)C * C, bpo, X, xbs, X, xbs, C, HW, B);
}

// TransformerBlock (:156-170) in place on X: x += project_out(attn(norm1(x))); x += ffn(norm2(x))
hipError_t block(xsd_restormer* r, hipStream_t s, const Blk& k, float* X, long long xbs, int H, int W)
{
    const int B = r->B, C = k.C, ln = r->cfg.layernorm_bias_free ? 2 : 1;
    const long long HW = (long long)H * W;
    hipError_t e;
    if ((e = pw(s, X, xbs, C, P(r, k.n1w), P(r, k.n1b), ln, r->wt + k.qkv.t, 0, P(r, k.qkv.b), nullptr, 0, r->Ta, 3 * C * HW, 3 * C, HW, B))) return e;
    if ((e = dw(s, r->Ta, 3 * C * HW, P(r, k.qkv_dw), P(r, k.qkv_dwb), r->Tb, 3 * C * HW, 3 * C, 0, H, W, B))) return e;
    if ((e = attention(s, r->Tb, 3 * C * HW, P(r, k.temp), r->wt + k.po.t, P(r, k.po.b), (double*)r->part, r->attn, r->mt, X, xbs, C, k.heads, HW, B))) return e;
    if ((e = pw(s, X, xbs, C, P(r, k.n2w), P(r, k.n2b), ln, r->wt + k.pin.t, 0, P(r, k.pin.b), nullptr, 0, r->Ta, 2 * k.hid * HW, 2 * k.hid, HW, B))) return e;
    if ((e = dw(s, r->Ta, 2 * k.hid * HW, P(r, k.ffn_dw), P(r, k.ffn_dwb), r->Tb, k.hid * HW, k.hid, 1, H, W, B))) return e;
    return pw(s, r->Tb, k.hid * HW, k.hid, nullptr, nullptr, 0, r->wt + k.pout.t, 0, P(r, k.pout.b), X, xbs, X, xbs, C, HW, B);
}

hipError_t blocks(xsd_restormer* r, hipStream_t s, const std::vector<Blk>& v, float* X, long long xbs, int H, int W)
{
    for (const Blk& k : v) {
        hipError_t e = block(r, s, k, X, xbs, H, W);
        if (e) return e;
    }
    return hipSuccess;
}

// workspace of one (B, H, W) in floats; with `assign` set, also the pointers into r->ws (a sizing call leaves the engine's plan alone)
long long plan_ws(xsd_restormer* r, int B, int H, int W, bool assign)
{
    const long long d = r->dim, HW1 = (long long)H * W, HW2 = HW1 / 4, HW3 = HW1 / 16, HW4 = HW1 / 64;
    long long t = 0, part = 0, mt = 0, attn = 0;
    auto level = [&](const std::vector<Blk>& v, long long HW) {
        for (const Blk& k : v) {
            t = std::max(t, std::max(3ll * k.C, 2ll * k.hid) * HW);
            part = std::max(part, (long long)k.heads * nsplit_of(HW, GRAM_CHUNK) * (k.ch * k.ch + 2 * k.ch));
            mt = std::max(mt, (long long)k.C * k.C);
            if (k.ch > AT_MAXCH) attn = std::max(attn, (long long)k.C * k.ch);       // the wide path's [heads][ch][ch]
        }
    };
    level(r->enc1, HW1); level(r->dec1, HW1); level(r->refine, HW1);
    level(r->enc2, HW2); level(r->dec2, HW2); level(r->enc3, HW3); level(r->dec3, HW3); level(r->lat, HW4);
    const long long sizes[11] = {B * 2 * d * HW1, B * 4 * d * HW2, B * 2 * d * HW2, B * 8 * d * HW3, B * 4 * d * HW3, B * 8 * d * HW4,
                                 B * t, B * t, 2 * B * part, B * mt, B * attn};      // (the Gram partials are doubles)
    float** ptrs[11] = {&r->slab1, &r->slab2, &r->dec2b, &r->slab3, &r->dec3b, &r->latb, &r->Ta, &r->Tb, &r->part, &r->mt, &r->attn};
    long long off = 0;
    for (int i = 0; i < 11; ++i) {
        if (assign) *ptrs[i] = (float*)r->ws + off;
        off += (sizes[i] + 63) / 64 * 64;        // 256-B aligned
    }
    return off;
}

} // namespace

extern "C" {

int xsd_restormer_create(const xsd_restormer_config* cfg, xsd_restormer** out)
{
    if (!cfg || !out) return rfail(XSD_ERR_ARG, "null argument");
    const auto& c = *cfg;
    if (c.dual_pixel_task) return rfail(XSD_ERR_ARG, "Restormer: dual_pixel_task is not supported by the MI355X engine");
    if (c.inp_channels < 1 || c.inp_channels > 1024 || c.out_channels != c.inp_channels)
        return rfail(XSD_ERR_ARG, "Restormer: `output(x) + inp_img` needs out_channels == inp_channels in [1, 1024] (got %d, %d)", c.inp_channels, c.out_channels);
    if (c.dim < 2 || c.dim > 1024 || c.dim % 2)
        return rfail(XSD_ERR_ARG, "Restormer: dim must be even and in [2, 1024] (Downsample halves it; got %d)", c.dim);
    for (int l = 0; l < 4; ++l) {
        if (c.num_blocks[l] < 0 || c.num_blocks[l] > 64) return rfail(XSD_ERR_ARG, "Restormer: num_blocks[%d] must be in [0, 64]", l);
        const int C = c.dim << l;
        if (c.heads[l] < 1 || C % c.heads[l]) return rfail(XSD_ERR_ARG, "Restormer: heads[%d] = %d does not divide the %d channels of level %d", l, c.heads[l], C, l + 1);
        if (C / c.heads[l] > WD_MAXCH) return rfail(XSD_ERR_ARG, "Restormer: %d channels per head at level %d; the engine takes at most %d", C / c.heads[l], l + 1, WD_MAXCH);
    }
    if (2 * c.dim / c.heads[0] > WD_MAXCH || (2 * c.dim) % c.heads[0])
        return rfail(XSD_ERR_ARG, "Restormer: heads[0] = %d must divide the %d decoder level-1 channels into at most %d per head", c.heads[0], 2 * c.dim, WD_MAXCH);
    if (c.num_refinement_blocks < 0 || c.num_refinement_blocks > 64) return rfail(XSD_ERR_ARG, "Restormer: num_refinement_blocks must be in [0, 64]");
    if (!(c.ffn_expansion_factor > 0) || hidden_of(c, c.dim) < 1 || (double)c.dim * 8 * c.ffn_expansion_factor > 65536)
        return rfail(XSD_ERR_ARG, "Restormer: ffn_expansion_factor %g gives no usable hidden width", c.ffn_expansion_factor);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rfail(XSD_ERR_HIP, "no HIP device available");
    xsd_restormer* r = new xsd_restormer();
    r->cfg = c;
    r->dim = c.dim;
    layout(r);
    if (xsd::dev_alloc((void**)&r->wt, sizeof(float) * std::max(1ll, r->wt_floats)) != hipSuccess) {
        (void)hipGetLastError();
        delete r;
        return rfail(XSD_ERR_NOMEM, "Restormer: packed-weight allocation failed");
    }
    *out = r;
    return XSD_OK;
}

void xsd_restormer_destroy(xsd_restormer* r) { delete r; }

int64_t xsd_restormer_param_count(const xsd_restormer* r) { return r ? r->nparams : -1; }

int xsd_restormer_pack_weights(xsd_restormer* r, const float* dev_params, void* stream)
{
    if (!r || !dev_params) return rfail(XSD_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    r->params = dev_params;
    for (const Pw1* p : r->pw1s) {
        const long long n = (long long)p->cout * p->cin;
        hipLaunchKernelGGL(rst_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dev_params + p->w, r->wt + p->t, p->cout, p->cin);
        hipError_t e = hipGetLastError();
        if (e) return rfail(XSD_ERR_HIP, "Restormer weight packing: %s", hipGetErrorString(e));
    }
    r->packed = true;
    return XSD_OK;
}

int xsd_restormer_forward(xsd_restormer* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream)
{
    if (!r || !dev_x || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "bad shape %dx%dx%d", B, H, W);
    if (H % 8 || W % 8)
        return rfail(XSD_ERR_ARG, "Restormer: H and W must be divisible by 8 (three PixelUnshuffle(2) levels); got %d x %d", H, W);
    if ((long long)H * W > (1ll << 28)) return rfail(XSD_ERR_ARG, "Restormer: image of %d x %d pixels is too large", H, W);
    if (!r->packed) return rfail(XSD_ERR_STATE, "xsd_restormer_pack_weights must be called before xsd_restormer_forward");
    hipStream_t s = (hipStream_t)stream;
    if (r->B != B || r->H != H || r->W != W) {
        const size_t need = sizeof(float) * (size_t)plan_ws(r, B, H, W, false) + 256;
        if (need > r->ws_bytes) {
            // refused BEFORE the held workspace is given up or anything is enqueued: the engine stays usable at its last shape
            const double gb = 1.0 / (1024.0 * 1024.0 * 1024.0);
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b + r->ws_bytes)
                return rfail(XSD_ERR_NOMEM, "Restormer: a workspace of %.1f GiB for %d x %d x %d tiles does not fit this device (%.1f GiB free + %.1f GiB held "
                             "by this engine of %.1f GiB); use a smaller batch per call", need * gb, B, H, W, free_b * gb, r->ws_bytes * gb, total_b * gb);
            if (r->ws) { hipDeviceSynchronize(); xsd::dev_free(r->ws); r->ws = nullptr; r->ws_bytes = 0; r->B = r->H = r->W = 0; }
            hipError_t err = xsd::dev_alloc((void**)&r->ws, need);
            if (err != hipSuccess) {
                (void)hipGetLastError();
                return rfail(XSD_ERR_NOMEM, "Restormer: workspace allocation (%.1f GiB for %d x %d x %d tiles) failed: %s", need * gb, B, H, W, hipGetErrorString(err));
            }
            r->ws_bytes = need;
        }
        plan_ws(r, B, H, W, true);
        r->B = B; r->H = H; r->W = W;
    }
    const auto& c = r->cfg;
    const long long d = r->dim, HW1 = (long long)H * W, HW2 = HW1 / 4, HW3 = HW1 / 16, HW4 = HW1 / 64;
    const int H2 = H / 2, W2 = W / 2, H3 = H / 4, W3 = W / 4, H4 = H / 8, W4 = W / 8;
    float* X1 = r->slab1 + d * HW1;            // encoder level 1 = upper half of the level-1 slab (the skip of torch.cat, :396)
    float* X2 = r->slab2 + 2 * d * HW2;
    float* X3 = r->slab3 + 4 * d * HW3;
    const long long s1 = 2 * d * HW1, s2 = 4 * d * HW2, s3 = 8 * d * HW3, s4 = 8 * d * HW4;
    hipError_t e = hipSuccess;
#define RST(x) do { if ((e = (x)) != hipSuccess) return rfail(XSD_ERR_HIP, "Restormer forward: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); } while (0)
    RST(conv3(s, dev_x, c.inp_channels * HW1, c.inp_channels, r->params + r->patch, nullptr, X1, s1, (int)d, H, W, 0, nullptr, 0, B));
    RST(blocks(r, s, r->enc1, X1, s1, H, W));
    RST(conv3(s, X1, s1, (int)d, r->params + r->down12, nullptr, X2, s2, (int)(d / 2), H, W, 1, nullptr, 0, B));
    RST(blocks(r, s, r->enc2, X2, s2, H2, W2));
    RST(conv3(s, X2, s2, (int)(2 * d), r->params + r->down23, nullptr, X3, s3, (int)d, H2, W2, 1, nullptr, 0, B));
    RST(blocks(r, s, r->enc3, X3, s3, H3, W3));
    RST(conv3(s, X3, s3, (int)(4 * d), r->params + r->down34, nullptr, r->latb, s4, (int)(2 * d), H3, W3, 1, nullptr, 0, B));
    RST(blocks(r, s, r->lat, r->latb, s4, H4, W4));
    RST(conv3(s, r->latb, s4, (int)(8 * d), r->params + r->up43, nullptr, r->slab3, s3, (int)(16 * d), H4, W4, 2, nullptr, 0, B));
    RST(pw(s, r->slab3, s3, (int)(8 * d), nullptr, nullptr, 0, r->wt + r->red3.t, 0, P(r, r->red3.b), nullptr, 0, r->dec3b, 4 * d * HW3, (int)(4 * d), HW3, B));
    RST(blocks(r, s, r->dec3, r->dec3b, 4 * d * HW3, H3, W3));
    RST(conv3(s, r->dec3b, 4 * d * HW3, (int)(4 * d), r->params + r->up32, nullptr, r->slab2, s2, (int)(8 * d), H3, W3, 2, nullptr, 0, B));
    RST(pw(s, r->slab2, s2, (int)(4 * d), nullptr, nullptr, 0, r->wt + r->red2.t, 0, P(r, r->red2.b), nullptr, 0, r->dec2b, 2 * d * HW2, (int)(2 * d), HW2, B));
    RST(blocks(r, s, r->dec2, r->dec2b, 2 * d * HW2, H2, W2));
    RST(conv3(s, r->dec2b, 2 * d * HW2, (int)(2 * d), r->params + r->up21, nullptr, r->slab1, s1, (int)(4 * d), H2, W2, 2, nullptr, 0, B));
    RST(blocks(r, s, r->dec1, r->slab1, s1, H, W));
    RST(blocks(r, s, r->refine, r->slab1, s1, H, W));
    RST(conv3(s, r->slab1, s1, (int)(2 * d), r->params + r->outw, P(r, r->outb), dev_y, c.out_channels * HW1, c.out_channels, H, W, 0, dev_x,
              c.inp_channels * HW1, B));
#undef RST
    return XSD_OK;
}

// ---- the kernels on their own (tests): see include/xsd.h ----------------------------------------------------------------------

namespace {

// what every hook's launch grid needs: the images go to gridDim.z, channel groups to gridDim.y
int check_grid(const char* what, int B, long long HW)
{
    if (B < 1 || B > 65535) return rfail(XSD_ERR_ARG, "%s: %d images are outside [1, 65535]", what, B);
    if (HW < 1 || HW > (1ll << 28)) return rfail(XSD_ERR_ARG, "%s: %lld pixels are outside [1, 2^28]", what, HW);
    return XSD_OK;
}

struct Scratch {                       // device allocations of one hook call
    std::vector<void*> ptrs;
    ~Scratch() { for (void* p : ptrs) xsd::dev_free(p); }
    void* get(size_t bytes)
    {
        void* p = nullptr;
        if (xsd::dev_alloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ptrs.push_back(p);
        return p;
    }
};

hipError_t transpose(hipStream_t s, const float* src, float* dst, int rows, int cols)
{
    const long long n = (long long)rows * cols;
    hipLaunchKernelGGL(rst_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows, cols);
    return hipGetLastError();
}

} // namespace

int xsd_restormer_test_pw(const float* dev_x, int64_t xbs, const float* dev_w, int per_image, const float* dev_bias, int ln, const float* dev_lnw,
                          const float* dev_lnb, int residual, float* dev_y, int64_t ybs, int B, int cin, int cout, int64_t HW, void* stream)
{
    if (!dev_x || !dev_w || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (int rc = check_grid("Restormer 1x1 test", B, HW)) return rc;
    if (cin < 1 || cin > 131072 || cout < 1 || cout > 131072)
        return rfail(XSD_ERR_ARG, "Restormer 1x1 test: %d -> %d channels are outside [1, 131072]", cin, cout);
    if (ln < 0 || ln > 2) return rfail(XSD_ERR_ARG, "Restormer 1x1 test: LayerNorm mode %d is not 0 (none), 1 (WithBias) or 2 (BiasFree)", ln);
    if ((ln && !dev_lnw) || (ln == 1 && !dev_lnb)) return rfail(XSD_ERR_ARG, "Restormer 1x1 test: LayerNorm mode %d needs its weight%s", ln, ln == 1 ? " and bias" : "");
    if (xbs < (int64_t)cin * HW || ybs < (int64_t)cout * HW)
        return rfail(XSD_ERR_ARG, "Restormer 1x1 test: batch strides %lld / %lld are smaller than the %d / %d channels of %lld pixels", (long long)xbs,
                     (long long)ybs, cin, cout, (long long)HW);
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    const int nw = per_image ? B : 1;
    const long long wn = (long long)cin * cout;
    float* wt = (float*)sc.get(sizeof(float) * (size_t)nw * wn);
    if (!wt) return rfail(XSD_ERR_NOMEM, "Restormer 1x1 test: allocation failed");
    hipError_t e = hipSuccess;
    for (int i = 0; i < nw && !e; ++i) e = transpose(s, dev_w + i * wn, wt + i * wn, cout, cin);
    if (!e) e = pw(s, dev_x, xbs, cin, dev_lnw, dev_lnb, ln, wt, per_image ? wn : 0, dev_bias, residual ? dev_y : nullptr, residual ? ybs : 0, dev_y, ybs,
                   cout, HW, B);
    hipStreamSynchronize(s);
    if (e) return rfail(XSD_ERR_HIP, "Restormer 1x1 test: %s", hipGetErrorString(e));
    return XSD_OK;
}

int xsd_restormer_test_dw(const float* dev_x, const float* dev_w, const float* dev_bias, float* dev_y, int B, int cout, int gate, int H, int W,
                          void* stream)
{
    if (!dev_x || !dev_w || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (H < 1 || W < 1) return rfail(XSD_ERR_ARG, "Restormer depthwise test: bad image size %d x %d", H, W);
    const long long HW = (long long)H * W;
    if (int rc = check_grid("Restormer depthwise test", B, HW)) return rc;
    if (cout < 1 || cout > 65535) return rfail(XSD_ERR_ARG, "Restormer depthwise test: %d output channels are outside [1, 65535]", cout);
    if (gate != 0 && gate != 1) return rfail(XSD_ERR_ARG, "Restormer depthwise test: mode %d is not 0 (plain) or 1 (gate)", gate);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = dw(s, dev_x, (gate ? 2 : 1) * cout * HW, dev_w, dev_bias, dev_y, cout * HW, cout, gate, H, W, B);
    hipStreamSynchronize(s);
    if (e) return rfail(XSD_ERR_HIP, "Restormer depthwise test: %s", hipGetErrorString(e));
    return XSD_OK;
}

namespace {

// both attention hooks: `wide` runs the wide kernels at any width they take, else attention() as the forward calls it, held to the
// narrow kernels' width
int test_attention(const char* what, bool wide, const float* dev_qkv, const float* dev_temperature, const float* dev_wpo, const float* dev_bpo,
                   float* dev_x, int B, int C, int heads, int64_t HW, void* stream)
{
    if (!dev_qkv || !dev_temperature || !dev_wpo || !dev_x) return rfail(XSD_ERR_ARG, "null argument");
    if (int rc = check_grid(what, B, HW)) return rc;
    if (heads < 1 || heads > 65535 || C < 1 || C % heads) return rfail(XSD_ERR_ARG, "%s: %d heads do not divide %d channels", what, heads, C);
    if (C / heads > (wide ? WD_MAXCH : AT_MAXCH))
        return rfail(XSD_ERR_ARG, "%s: %d channels per head; the %skernels take at most %d", what, C / heads, wide ? "wide " : "", wide ? WD_MAXCH : AT_MAXCH);
    if (C > 8192) return rfail(XSD_ERR_ARG, "%s: %d channels are outside [1, 8192]", what, C);
    hipStream_t s = (hipStream_t)stream;
    const int ch = C / heads;
    Scratch sc;
    float* wt = (float*)sc.get(sizeof(float) * (size_t)C * C);
    float* mt = (float*)sc.get(sizeof(float) * (size_t)B * C * C);
    float* attn = wide ? (float*)sc.get(sizeof(float) * (size_t)B * C * ch) : nullptr;
    double* part = (double*)sc.get(sizeof(double) * (size_t)B * heads * nsplit_of(HW, GRAM_CHUNK) * (ch * ch + 2 * ch));
    if (!wt || !mt || !part || (wide && !attn)) return rfail(XSD_ERR_NOMEM, "%s: allocation failed", what);
    hipError_t e = transpose(s, dev_wpo, wt, C, C);
    if (!e) e = (wide ? attention_wide : attention)(s, dev_qkv, 3 * C * HW, dev_temperature, wt, dev_bpo, part, attn, mt, dev_x, C * HW, C, heads, HW, B);
    hipStreamSynchronize(s);
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return XSD_OK;
}

} // namespace

int xsd_restormer_test_attention(const float* dev_qkv, const float* dev_temperature, const float* dev_wpo, const float* dev_bpo, float* dev_x, int B,
                                 int C, int heads, int64_t HW, void* stream)
{
    return test_attention("Restormer attention test", false, dev_qkv, dev_temperature, dev_wpo, dev_bpo, dev_x, B, C, heads, HW, stream);
}

int xsd_restormer_test_attention_wide(const float* dev_qkv, const float* dev_temperature, const float* dev_wpo, const float* dev_bpo, float* dev_x,
                                      int B, int C, int heads, int64_t HW, void* stream)
{
    return test_attention("Restormer wide attention test", true, dev_qkv, dev_temperature, dev_wpo, dev_bpo, dev_x, B, C, heads, HW, stream);
}

int xsd_restormer_test_conv3(const float* dev_x, const float* dev_w, const float* dev_bias, const float* dev_skip, float* dev_y, int B, int cin,
                             int cout, int H, int W, int mode, void* stream)
{
    if (!dev_x || !dev_w || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (H < 1 || W < 1) return rfail(XSD_ERR_ARG, "Restormer 3x3 test: bad image size %d x %d", H, W);
    const long long HW = (long long)H * W;
    if (int rc = check_grid("Restormer 3x3 test", B, HW)) return rc;
    if (cin < 1 || cin > 131072 || cout < 1 || cout > 131072)
        return rfail(XSD_ERR_ARG, "Restormer 3x3 test: %d -> %d channels are outside [1, 131072]", cin, cout);
    if (mode < 0 || mode > 2) return rfail(XSD_ERR_ARG, "Restormer 3x3 test: mode %d is not 0 (plain), 1 (PixelUnshuffle) or 2 (PixelShuffle)", mode);
    if (mode == 1 && (H % 2 || W % 2)) return rfail(XSD_ERR_ARG, "Restormer 3x3 test: PixelUnshuffle(2) needs even H and W; got %d x %d", H, W);
    if (mode == 2 && cout % 4) return rfail(XSD_ERR_ARG, "Restormer 3x3 test: PixelShuffle(2) needs a multiple of 4 output channels; got %d", cout);
    if (mode != 0 && dev_skip) return rfail(XSD_ERR_ARG, "Restormer 3x3 test: the skip is added in the plain mode only");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = conv3(s, dev_x, cin * HW, cin, dev_w, dev_bias, dev_y, cout * HW, cout, H, W, mode, dev_skip, cout * HW, B);
    hipStreamSynchronize(s);
    if (e) return rfail(XSD_ERR_HIP, "Restormer 3x3 test: %s", hipGetErrorString(e));
    return XSD_OK;
}

} // extern "C"
