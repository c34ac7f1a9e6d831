// sw_kernels.h -- the exact-fp32 kernels that the Swin-family networks (swinfir.hip, hat.hip, swinir.hip) share, with their launch helpers.
//
// Every product is an fp32 FMA on the fp32 matrix instruction v_mfma_f32_32x32x2_f32 (bitwise a k-ordered fmaf chain).  The GEMM's
// fmaf chains are 16 long (4 where K <= 48), their sums over K are carried in double, as are the LayerNorm statistics.  No float atomics anywhere and
// every reduction has a fixed order: an image's output is bitwise independent of the batch it shares and of the run.
//
// Feature maps are TOKEN-MAJOR ([B][H*W][C], C contiguous): the Swin blocks' (B, L, C) layout, and at the same time the NHWC view
// that the 3x3 convs read and write through their addressing.
//
// Kernels:
//   sw_gemm_kernel   C = A W (+ bias) on MFMA, 128 x 64 tile per workgroup.  A is either token rows (a Linear / 1x1 conv) or the
//                    implicit im2col of a 3x3 conv (zero pad 1; NCHW or token-major input, with
//                    the input affine (x - mean) * img_range of conv_first).  Epilogue: exact-erf GELU or LeakyReLU, residual add
//                    (may alias the output), and a token-major, PixelShuffle(r) or NCHW (x / img_range + mean) store.
//   sw_attn_kernel   one workgroup per (window, head): softmax(q scale k^T + table[index] (+ the -100 shift mask)) v, reading q, k,
//                    v from the qkv rows through the roll / window-partition addressing and writing the same way back.
//   sw_ln_kernel     LayerNorm over the channels of each token (norm1 / norm2 in front of qkv / fc1, patch_embed.norm, the final
//                    norm), one wave per token, statistics in double.
//   sw_pack_kernel   a Linear / conv weight as stored -> the [K][N] matrix sw_gemm_kernel reads.
//
// The opt-in bf16x6 math mode runs the GEMM on sw_gemm_s3x.h's kernel instead; everything here stays exact fp32 in every mode.
//
// Everything is in an anonymous namespace: each including file compiles its own instance.
#ifndef XSD_SW_KERNELS_H
#define XSD_SW_KERNELS_H
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

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------
constexpr int GM = 128;      // rows (tokens / pixels) per workgroup: wave w owns rows [32 w, 32 w + 32)
constexpr int GN = 64;       // output columns per workgroup: two 32 x 32 accumulators per wave
constexpr int GK = 16;       // K per LDS round
constexpr int GAP = GM + 4;  // LDS row pitch of the A tile
constexpr int GK_SHORT = 3 * GK;   // a sum of at most this many terms runs in fmaf chains of 4 instead of 16 (sw_gemm_kernel)

enum { A_TOK = 0, A_CONV3 = 1 };
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_LRELU = 2 };
enum { O_TOK = 0, O_SHUFFLE = 1, O_NCHW = 2, O_SHUFFLE_NCHW = 3 };

// The addressing that only SwinIR uses (GemmP's last fields: the nearest-2x source of a conv, an NCHW residual, cropped NCHW stores,
// PixelShuffle straight into NCHW) is compiled into the GEMM kernels of a file that defines SW_GEMM_EXT as 1 before it includes this
// header.  The other files' instances are built without it: the instruction streams of SwinFIR and HAT hold none of it.
#ifndef SW_GEMM_EXT
#define SW_GEMM_EXT 0
#endif

struct GemmP {
    int amode;
    const float* a; long long abs, acs, aps;   // element (b, channel k or ci, row p) at a + b abs + k acs + p aps
    int K, cin;                                // token: K = cin; conv: K = 9 cin, k = tap * cin + ci
    int B, H, W; long long HW;                 // images; rows per image (conv: H W)
    const float* isub; float imul;             // conv mode: (x - isub[ci]) * imul inside the image, or null
    const float* w; int N;                     // packed [K][N]
    const float* bias;                         // [N] or null
    int act; float slope;
    const float* res; long long rbs, rps;      // v += res[b rbs + p rps + n] (may alias y: same element, same thread) or null
    int omode;
    float* y; long long ybs, yps;              // O_TOK: y[b ybs + p yps + n]; O_SHUFFLE: yps = N / r^2 channels of the r H x r W output
    int r;
    const float* omean; float orange;          // O_NCHW: y[b ybs + n HW + p] = v / orange + omean[n]
    // SW_GEMM_EXT only; all zero = none of it
    int up2;                                   // conv mode: the input is the nearest-2x upsampling of an (H / 2) x (W / 2) image that is never
                                               // made: tap (yy, xx) of the H x W extent (which the zero padding is tested against) reads
                                               // source pixel (yy >> 1, xx >> 1); abs is the stride of a SOURCE image
    int rnchw;                                 // the residual is NCHW: res[b rbs + n HW + p]
    int cH, cW;                                // O_NCHW: only rows < cH and columns < cW are stored, as a [N][cH][cW] image at b ybs.
                                               // O_SHUFFLE_NCHW: PixelShuffle(r) of the N = r^2 channels-out columns, v / orange + omean[ch],
                                               // into the [N / r^2][cH][cW] image at b ybs (the crop of the r H x r W result)
};

// SW_GEMM_EXT_SRC(yy, xx): the source pixel of tap (yy, xx) inside the image
#if SW_GEMM_EXT
#define SW_GEMM_EXT_SRC(yy, xx) (P.up2 ? (long long)((yy) >> 1) * (P.W >> 1) + ((xx) >> 1) : (long long)(yy) * P.W + (xx))

// the residual add and the store of one result with the SwinIR addressing: the epilogue tail of both GEMM kernels of such a file
__device__ __forceinline__ void gemm_store_ext(const GemmP& P, float x, long long b, long long p, int n)
{
    if (P.res) x += P.rnchw ? P.res[b * P.rbs + (long long)n * P.HW + p] : P.res[b * P.rbs + p * P.rps + n];
    if (P.omode == O_TOK) {
        P.y[b * P.ybs + p * P.yps + n] = x;
    } else if (P.omode == O_SHUFFLE) {
        const int r = P.r, ch = n / (r * r), rem = n - ch * r * r, ii = rem / r, jj = rem - ii * r;
        const long long py = p / P.W, px = p - py * P.W;
        P.y[b * P.ybs + ((py * r + ii) * ((long long)P.W * r) + px * r + jj) * P.yps + ch] = x;
    } else if (P.omode == O_SHUFFLE_NCHW) {
        const int r = P.r, ch = n / (r * r), rem = n - ch * r * r, ii = rem / r, jj = rem - ii * r;
        const long long py = p / P.W, px = p - py * P.W, oy = py * r + ii, ox = px * r + jj;
        if (oy < P.cH && ox < P.cW) P.y[b * P.ybs + ((long long)ch * P.cH + oy) * P.cW + ox] = x / P.orange + P.omean[ch];
    } else if (P.cW) {
        const long long py = p / P.W, px = p - py * P.W;
        if (py < P.cH && px < P.cW) P.y[b * P.ybs + ((long long)n * P.cH + py) * P.cW + px] = x / P.orange + P.omean[n];
    } else {
        P.y[b * P.ybs + (long long)n * P.HW + p] = x / P.orange + P.omean[n];
    }
}
#else
#define SW_GEMM_EXT_SRC(yy, xx) ((long long)yy * P.W + xx)
#endif

template <bool SHORTK>      // SHORTK: K <= GK_SHORT (gemm() picks the instance)
__global__ __launch_bounds__(256) void sw_gemm_kernel(const GemmP P)
{
    __shared__ __attribute__((aligned(16))) float As[GK][GAP];
    __shared__ __attribute__((aligned(16))) float Bs[GK][GN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long M = (long long)P.B * P.HW;
    const long long m0 = (long long)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;

    // the rows this thread stages: ml = (tid >> 4) + 16 i, at k = k0 + (tid & 15)
    const int kl = tid & 15;
    long long rbase[8];
    int ry[8], rx[8];
    bool rok[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long long m = m0 + (tid >> 4) + 16 * i;
        rok[i] = m < M;
        const long long b = rok[i] ? m / P.HW : 0, p = rok[i] ? m - b * P.HW : 0;
        rbase[i] = b * P.abs + (P.amode == A_TOK ? p * P.aps : 0);
        ry[i] = P.amode == A_CONV3 ? (int)(p / P.W) : 0;
        rx[i] = P.amode == A_CONV3 ? (int)(p - (long long)ry[i] * P.W) : 0;
    }

    float av[8], bv[4];
    auto load = [&](int k0) {
        const int k = k0 + kl;
        if (P.amode == A_TOK) {
            const bool kok = k < P.K;
#pragma unroll
            for (int i = 0; i < 8; ++i) av[i] = (rok[i] && kok) ? P.a[rbase[i] + (long long)k * P.acs] : 0.f;
        } else {
            const bool kok = k < P.K;
            const int tap = kok ? k / P.cin : 0, ci = kok ? k - tap * P.cin : 0;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            const float sub = (P.isub && kok) ? P.isub[ci] : 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int yy = ry[i] + dy, xx = rx[i] + dx;
                float v = 0.f;
                if (rok[i] && kok && yy >= 0 && yy < P.H && xx >= 0 && xx < P.W) {
                    v = P.a[rbase[i] + (long long)ci * P.acs + SW_GEMM_EXT_SRC(yy, xx) * P.aps];
                    if (P.isub) v = (v - sub) * P.imul;
                }
                av[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = k0 + (tid >> 6) + 4 * i, n = n0 + (tid & 63);
            bv[i] = (kk < P.K && n < P.N) ? P.w[(long long)kk * P.N + n] : 0.f;
        }
    };

    // each K round is a 16-term fmaf chain on the MFMA from zero; the rounds are summed in double (a fixed order).  A sum of at most
    // GK_SHORT terms (conv_first from 1 to 5 channels, layers narrower than any published embed_dim) is cut into chains of 4 instead:
    // there a correctly rounded sum is what the chain's roundings are measured against (at K = 36 chains of 16 left 2.5 x its
    // max-relative error), and the four flushes per round are paid for three rounds at most.  Longer sums keep their bits and speed.
    double d0[16], d1[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) { d0[v] = 0.0; d1[v] = 0.0; }
    const int i32 = lane & 31, h2 = lane >> 5;
    f32x16 acc0, acc1;
    // steps [s0, s1) of a round as one chain from zero, added to the double sums
    auto chain = [&](const int s0, const int s1) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
#pragma unroll
        for (int s = s0; s < s1; ++s) {
            const float a = As[2 * s + h2][32 * wave + i32];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[2 * s + h2][i32], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[2 * s + h2][32 + i32], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) { d0[v] += (double)acc0[v]; d1[v] += (double)acc1[v]; }
    };
    load(0);
    for (int k0 = 0; k0 < P.K; k0 += GK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) As[kl][(tid >> 4) + 16 * i] = av[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[(tid >> 6) + 4 * i][tid & 63] = bv[i];
        __syncthreads();
        if (k0 + GK < P.K) load(k0 + GK);
        if (SHORTK) {
#pragma unroll
            for (int s = 0; s < GK / 2; s += 2) chain(s, s + 2);
        } else {
            chain(0, GK / 2);
        }
    }
    // accumulator register v of lane l: row 32 wave + 8 (v / 4) + 4 (l / 32) + v % 4, column 32 c + l % 32
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n = n0 + 32 * c + i32;
        if (n >= P.N) continue;
        const float bn = P.bias ? P.bias[n] : 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long long m = m0 + 32 * wave + 8 * (v >> 2) + 4 * h2 + (v & 3);
            if (m >= M) continue;
            // SW_GEMM_EXT: the bias joins the double sum, so the result is rounded to fp32 once.  The other instances keep their two
            // roundings (sum, then + bias): their outputs stay what they were, bit for bit.
#if SW_GEMM_EXT
            float x = (float)((c ? d1[v] : d0[v]) + (double)bn);
#else
            float x = (float)(c ? d1[v] : d0[v]) + bn;
#endif
            if (P.act == ACT_GELU) x = 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
            else if (P.act == ACT_LRELU) x = x >= 0.f ? x : x * P.slope;
            const long long b = m / P.HW, p = m - b * P.HW;
#if SW_GEMM_EXT
            gemm_store_ext(P, x, b, p, n);
#else
            if (P.res) x += P.res[b * P.rbs + p * P.rps + n];
            if (P.omode == O_TOK) {
                P.y[b * P.ybs + p * P.yps + n] = x;
            } else if (P.omode == O_SHUFFLE) {
                const int r = P.r, ch = n / (r * r), rem = n - ch * r * r, ii = rem / r, jj = rem - ii * r;
                const long long py = p / P.W, px = p - py * P.W;
                P.y[b * P.ybs + ((py * r + ii) * ((long long)P.W * r) + px * r + jj) * P.yps + ch] = x;
            } else {
                P.y[b * P.ybs + (long long)n * P.HW + p] = x / P.orange + P.omean[n];
            }
#endif
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// window attention
// ---------------------------------------------------------------------------------------------------------------
struct AttnP {
    const float* qkv;            // token rows of 3 C: q, k, v; head h at channels h hd .. h hd + hd - 1 of each (modules.py:115-125)
    float* o;                    // token rows of C
    const float* table;          // relative_position_bias_table [(2 ws - 1)^2][heads]
    int H, W, C, heads, hd, ws, shift, nwx, nw;
    float scale;
};

__device__ __forceinline__ int region(int r, int n, int ws, int s) { return r < n - ws ? 0 : (r < n - s ? 1 : 2); }

// NT 32-token tiles cover the ws^2 tokens of a window; wave w takes the queries [32 w, 32 w + 32).  Per wave the scores are
// computed TRANSPOSED, S^T = K (q scale)^T, so that lane l holds query l % 32 against 16 NT keys: the softmax over keys is a
// per-lane reduction plus one exchange with lane l ^ 32, and the probabilities are already the A operand of P V.
template <int NT>
__global__ __launch_bounds__(64 * NT) void sw_attn_kernel(const AttnP P)
{
    __shared__ float Ks[NT * 32][33];
    __shared__ float Vs[NT * 32][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i32 = lane & 31, h2 = lane >> 5;
    const int ws = P.ws, N = ws * ws, h = blockIdx.y;
    const int b = (int)blockIdx.x / P.nw, win = (int)blockIdx.x - b * P.nw;
    const int wy = win / P.nwx, wx = win - wy * P.nwx;
    const long long HW = (long long)P.H * P.W;
    const int C3 = 3 * P.C;
    auto tok = [&](int i) -> long long {       // window-local token -> row (roll by -shift, window_partition; modules.py:316-331)
        const int iy = i / ws, ix = i - iy * ws;
        const int y = (wy * ws + iy + P.shift) % P.H, x = (wx * ws + ix + P.shift) % P.W;
        return (long long)b * HW + (long long)y * P.W + x;
    };
    for (int e = tid; e < NT * 32 * 32; e += 64 * NT) {
        const int j = e >> 5, d = e & 31;
        float kv = 0.f, vv = 0.f;
        if (j < N && d < P.hd) {
            const float* row = P.qkv + tok(j) * C3 + h * P.hd + d;
            kv = row[P.C];
            vv = row[2 * P.C];
        }
        Ks[j][d] = kv;
        Vs[j][d] = vv;
    }
    const int qi = 32 * wave + i32;
    const bool qok = qi < N;
    float qv[16];
    {
        const float* row = P.qkv + (qok ? tok(qi) : 0) * C3 + h * P.hd;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int d = 2 * s + h2;
            qv[s] = (qok && d < P.hd) ? row[d] * P.scale : 0.f;        // q *= scale (modules.py:127)
        }
    }
    __syncthreads();
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (2 * s >= P.hd) break;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[32 * t + i32][2 * s + h2], qv[s], acc[t], 0, 0, 0);
        }
    }
    // acc[t][v] of lane l = S[query 32 wave + l % 32][key j = 32 t + 8 (v / 4) + 4 (l / 32) + v % 4]
    const int qy = qi / ws, qx = qi - (qi / ws) * ws, side = 2 * ws - 1;
    const int qreg = P.shift ? 3 * region(wy * ws + qy, P.H, ws, P.shift) + region(wx * ws + qx, P.W, ws, P.shift) : 0;
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int j = 32 * t + 8 * (v >> 2) + 4 * h2 + (v & 3);
            float s = acc[t][v];
            if (j >= N) s = -INFINITY;
            else if (qok) {
                const int ky = j / ws, kx = j - ky * ws;
                s += P.table[((qy - ky + ws - 1) * side + (qx - kx + ws - 1)) * P.heads + h];
                if (P.shift) {
                    const int kreg = 3 * region(wy * ws + ky, P.H, ws, P.shift) + region(wx * ws + kx, P.W, ws, P.shift);
                    if (kreg != qreg) s += -100.f;                    // the attn_mask of modules.py:268-297
                }
            }
            acc[t][v] = s;
            mx = fmaxf(mx, s);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float e = expf(acc[t][v] - mx);
            acc[t][v] = e;
            den += e;
        }
    den += __shfl_xor(den, 32);
    f32x16 o;
#pragma unroll
    for (int v = 0; v < 16; ++v) o[v] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v)
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[t][v] / den, Vs[32 * t + 8 * (v >> 2) + 4 * h2 + (v & 3)][i32], o, 0, 0, 0);
    // o[v] of lane l = out[query 32 wave + 8 (v / 4) + 4 (l / 32) + v % 4][d = l % 32]
    if (i32 >= P.hd) return;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int q = 32 * wave + 8 * (v >> 2) + 4 * h2 + (v & 3);
        if (q < N) P.o[tok(q) * P.C + h * P.hd + i32] = o[v];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm, weight packing
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sw_ln_kernel(const float* x, float* y, const float* w, const float* bias, long long M, int C)
{
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const float* xr = x + m * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)xr[c];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    const double mu = s / C;
    double q = 0.0;
    for (int c = lane; c < C; c += 64) { const double d = (double)xr[c] - mu; q = fma(d, d, q); }
    for (int o = 32; o; o >>= 1) q += __shfl_xor(q, o);
    const float muf = (float)mu, sd = (float)sqrt(q / C + 1e-5);
    for (int c = lane; c < C; c += 64) y[m * C + c] = (xr[c] - muf) / sd * w[c] + bias[c];
}

// [cout][cin][taps] (Linear / 1x1 / 3x3 weights) -> [taps][cin][cout] = the [K][N] sw_gemm_kernel reads
__global__ __launch_bounds__(256) void sw_pack_kernel(const float* src, float* dst, int cout, int cin, int taps)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)cout * cin * taps) return;
    const int co = (int)(i % cout);
    const long long r = i / cout;
    const int ci = (int)(r % cin), t = (int)(r / cin);
    dst[i] = src[((long long)co * cin + ci) * taps + t];
}

struct Lin { long long w = -1, b = -1, t = -1, t3 = -1; int cout = 0, cin = 0, taps = 1; };   // flat offsets of weight / bias, packed copy, bf16x6 planes

long long add(long long& off, long long n) { const long long o = off; off += n; return o; }

void lin(Lin& l, long long& off, int cout, int cin, int taps, bool bias)
{
    l.cout = cout; l.cin = cin; l.taps = taps;
    l.w = add(off, (long long)cout * cin * taps);
    l.b = bias ? add(off, cout) : -1;
}

int up_stages(int s) { return s == 3 ? 1 : (int)std::lround(std::log2((double)s)); }
int up_factor(int s) { return s == 3 ? 3 : 2; }

GemmP gp_tok(const float* a, long long rows, int K, long long lda, const float* w, int N, const float* bias, float* y, long long ldy)
{
    GemmP p{};
    p.amode = A_TOK; p.a = a; p.abs = 0; p.acs = 1; p.aps = lda; p.K = K; p.cin = K;
    p.B = 1; p.H = 1; p.W = (int)std::min<long long>(rows, 1 << 30); p.HW = rows;
    p.w = w; p.N = N; p.bias = bias; p.act = ACT_NONE; p.slope = 0.f;
    p.omode = O_TOK; p.y = y; p.ybs = 0; p.yps = ldy; p.r = 1; p.orange = 1.f;
    return p;
}

// a 3x3 conv over B images of H x W with cin token-major channels (x + b H W cin + p cin + ci) into a token-major output
GemmP gp_conv(const float* x, int B, int H, int W, int cin, const float* w, int N, const float* bias, float* y, long long ldy)
{
    GemmP p{};
    p.amode = A_CONV3; p.a = x; p.abs = (long long)H * W * cin; p.acs = 1; p.aps = cin; p.K = 9 * cin; p.cin = cin;
    p.B = B; p.H = H; p.W = W; p.HW = (long long)H * W;
    p.w = w; p.N = N; p.bias = bias; p.act = ACT_NONE; p.slope = 0.f;
    p.omode = O_TOK; p.y = y; p.ybs = p.HW * ldy; p.yps = ldy; p.r = 1; p.orange = 1.f;
    return p;
}

// a 3x3 conv over the nearest-2x upsampling of B token-major images of H x W (SW_GEMM_EXT): output rows are the 2 H x 2 W pixels
GemmP gp_conv_up2(const float* x, int B, int H, int W, int cin, const float* w, int N, const float* bias, float* y, long long ldy)
{
    GemmP p = gp_conv(x, B, 2 * H, 2 * W, cin, w, N, bias, y, ldy);
    p.abs = (long long)H * W * cin;
    p.up2 = 1;
    return p;
}

hipError_t gemm(hipStream_t s, const GemmP& p)
{
    const long long M = (long long)p.B * p.HW;
    dim3 grid((unsigned)((M + GM - 1) / GM), (unsigned)((p.N + GN - 1) / GN));
    // two instances, so that the long sums run the instruction stream they always ran
    if (p.K <= GK_SHORT) hipLaunchKernelGGL(sw_gemm_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(sw_gemm_kernel<false>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t ln(hipStream_t s, const float* x, float* y, const float* w, const float* b, long long M, int C)
{
    hipLaunchKernelGGL(sw_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, y, w, b, M, C);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// host side: what the engines of both networks hold and do alike
// ---------------------------------------------------------------------------------------------------------------
// `lins` holds pointers into the object that derives from this: such objects live on the heap only and are never copied.
struct SwBase {
    int E = 0, hid = 0, ws = 0, nfeat = 64;
    long long nparams = 0, wt_floats = 0;
    long long pen_w = -1, pen_b = -1, norm_w = 0, norm_b = 0;
    Lin first_l, after, before, last;
    std::vector<Lin> ups;
    std::vector<Lin*> lins;           // every weight the GEMM reads, in the order of the packed copy
    float* wt = nullptr;              // the packed copy
    int math = 0;                     // 0 = fp32, 3 = bf16x6 (sw_gemm_s3x.h): which kernel the forward's GEMMs run on
    unsigned short* wt3 = nullptr;    // bf16x6: the three bf16 planes of every weight, allocated when the mode is first used
    bool packed3 = false;             // wt3 follows the last pack_weights
    float* mean = nullptr;
    const float* params = nullptr;
    bool packed = false;
    int B = 0, H = 0, W = 0;          // the shape the workspace is planned for
    char* ws_buf = nullptr;
    size_t ws_bytes = 0;
    float *XF = nullptr, *X = nullptr, *A = nullptr, *O = nullptr, *V = nullptr, *U0 = nullptr, *U1 = nullptr, *R0 = nullptr;

    SwBase() = default;
    SwBase(const SwBase&) = delete;
    SwBase& operator=(const SwBase&) = delete;
    ~SwBase()
    {
        if (wt) xsd::dev_free(wt);
        if (wt3) xsd::dev_free(wt3);
        if (mean) xsd::dev_free(mean);
        if (ws_buf) xsd::dev_free(ws_buf);
    }
};

// the GEMM in the engine's math mode (sw_gemm_s3x.h); every GEMM of a forward goes through it
hipError_t gemm(hipStream_t s, const SwBase* r, const GemmP& p);

const float* PP(const SwBase* r, long long off) { return off < 0 ? nullptr : r->params + off; }

const char* upsampler_name(int u)
{
    switch (u) { case 0: return "pixelshuffle"; case 1: return "pixelshuffledirect"; case 2: return "nearest+conv"; default: return "\"\" (none)"; }
}

// the checks of the constructor arguments that both networks share, under the name `net` of the one that asks
// (upscale 1, a head that does not enlarge, is SwinIR's alone: `upscale1`)
template <class Cfg>
int check_dims(const Cfg& c, const char* net, bool upscale1 = false)
{
    if (c.in_chans < 1 || c.in_chans > 64) return rfail(XSD_ERR_ARG, "%s: in_chans must be in [1, 64] (got %d)", net, c.in_chans);
    if (c.embed_dim < 2 || c.embed_dim > 4096) return rfail(XSD_ERR_ARG, "%s: embed_dim must be in [2, 4096] (got %d)", net, c.embed_dim);
    if (c.num_layers < 0 || c.num_layers > 16) return rfail(XSD_ERR_ARG, "%s: at most 16 layers (got %d)", net, c.num_layers);
    if (c.upscale != 2 && c.upscale != 3 && c.upscale != 4 && c.upscale != 8 && !(upscale1 && c.upscale == 1))
        return rfail(XSD_ERR_ARG, "%s: upscale %d is not supported (2^n and 3, modules.py Upsample)", net, c.upscale);
    if (!(c.img_range > 0)) return rfail(XSD_ERR_ARG, "%s: img_range must be positive", net);
    if (!(c.qk_scale >= 0))
        return rfail(XSD_ERR_ARG, "%s: qk_scale %g is not supported (None / 0 for head_dim^-0.5, or a positive scale)", net, c.qk_scale);
    if (!(c.mlp_ratio > 0) || (int)(c.embed_dim * c.mlp_ratio) < 1 || c.embed_dim * c.mlp_ratio > 65536)
        return rfail(XSD_ERR_ARG, "%s: mlp_ratio %g gives no usable hidden width", net, c.mlp_ratio);
    if (c.img_size[0] < 1 || c.img_size[1] < 1 || c.patch_size[0] < 1 || c.patch_size[1] < 1 || c.window_size < 1)
        return rfail(XSD_ERR_ARG, "%s: img_size, patch_size and window_size must be positive", net);
    return XSD_OK;
}

template <class Cfg>
int check_layers(const Cfg& c, const char* net)
{
    for (int l = 0; l < c.num_layers; ++l) {
        if (c.depths[l] < 0 || c.depths[l] > 64) return rfail(XSD_ERR_ARG, "%s: depths[%d] must be in [0, 64]", net, l);
        const int h = c.num_heads[l];
        if (h < 1 || c.embed_dim % h) return rfail(XSD_ERR_ARG, "%s: num_heads[%d] = %d does not divide embed_dim %d", net, l, h, c.embed_dim);
        if (c.embed_dim / h > 32) return rfail(XSD_ERR_ARG, "%s: head dim %d at layer %d; the engine takes at most 32", net, c.embed_dim / h, l);
    }
    return XSD_OK;
}

// the packed copy of the weights and the per-channel mean of the input; on failure the caller deletes the engine
int alloc_weights(SwBase* r, const char* net, const std::vector<float>& mean)
{
    if (xsd::dev_alloc((void**)&r->wt, sizeof(float) * std::max(1ll, r->wt_floats)) != hipSuccess ||
        xsd::dev_alloc((void**)&r->mean, sizeof(float) * mean.size()) != hipSuccess ||
        hipMemcpy(r->mean, mean.data(), sizeof(float) * mean.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {      // (stream 0's upload is on the device before a forward on a non-blocking stream reads it)
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "%s: packed-weight allocation failed", net);
    }
    return XSD_OK;
}

int pack_weights(SwBase* r, const char* net, const float* dev_params, void* stream)
{
    if (!r || !dev_params) return rfail(XSD_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    r->params = dev_params;
    for (const Lin* p : r->lins) {
        const long long n = (long long)p->cout * p->cin * p->taps;
        hipLaunchKernelGGL(sw_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dev_params + p->w, r->wt + p->t, p->cout, p->cin, p->taps);
        hipError_t e = hipGetLastError();
        if (e) return rfail(XSD_ERR_HIP, "%s weight packing: %s", net, hipGetErrorString(e));
    }
    r->packed = true;
    r->packed3 = false;               // the bf16x6 planes are made again before the next forward that needs them
    return XSD_OK;
}

// makes the workspace hold `floats` floats for B tiles of H x W.  The caller then assigns its pointers and sets r->B / H / W.
int grow_ws(SwBase* r, const char* net, long long floats, int B, int H, int W)
{
    const size_t need = sizeof(float) * (size_t)floats + 256;
    if (need <= r->ws_bytes) return XSD_OK;
    // refused BEFORE the held workspace is given up or anything is enqueued: the engine stays usable at its last shape
    const double gb = 1.0 / (1024.0 * 1024.0 * 1024.0);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b + r->ws_bytes)
        return rfail(XSD_ERR_NOMEM, "%s: a workspace of %.1f GiB for %d x %d x %d tiles does not fit this device (%.1f GiB free + %.1f GiB held "
                     "by this engine of %.1f GiB); use a smaller batch per call", net, need * gb, B, H, W, free_b * gb, r->ws_bytes * gb, total_b * gb);
    if (r->ws_buf) { hipDeviceSynchronize(); xsd::dev_free(r->ws_buf); r->ws_buf = nullptr; r->ws_bytes = 0; r->B = r->H = r->W = 0; }
    hipError_t err = xsd::dev_alloc((void**)&r->ws_buf, need);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "%s: workspace allocation (%.1f GiB for %d x %d x %d tiles) failed: %s", net, need * gb, B, H, W, hipGetErrorString(err));
    }
    r->ws_bytes = need;
    return XSD_OK;
}

float attn_scale(double qk_scale, int hd) { return qk_scale > 0 ? (float)qk_scale : (float)std::pow((double)hd, -0.5); }   // `qk_scale or head_dim ** -0.5`

// qkv: token rows of 3 E (the qkv GEMM's output), out: token rows of E.  Both are passed by the caller: the forward's X / O roles
// change between layers (1conv swaps them), so nothing here may assume which workspace buffer holds what.  With a shift, the -100
// mask is the one of the run-time size.
hipError_t attention(hipStream_t s, const float* qkv, float* out, const float* table, int B, int H, int W, int E, int heads, int ws, int shift,
                     float scale)
{
    AttnP p{};
    p.qkv = qkv; p.o = out; p.table = table;
    p.H = H; p.W = W; p.C = E; p.heads = heads; p.hd = E / heads; p.ws = ws; p.shift = shift;
    p.nwx = W / ws; p.nw = (H / ws) * p.nwx;
    p.scale = scale;
    dim3 grid((unsigned)(B * p.nw), (unsigned)heads);
    const int nt = (ws * ws + 31) / 32;
    switch (nt) {
#define SW_ATT(T) case T: hipLaunchKernelGGL(sw_attn_kernel<T>, grid, dim3(64 * T), 0, s, p); break;
    SW_ATT(1) SW_ATT(2) SW_ATT(3) SW_ATT(4) SW_ATT(5) SW_ATT(6) SW_ATT(7) SW_ATT(8)
#undef SW_ATT
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// conv_first over (x - mean) * img_range, NCHW in, into XF; then patch_embed's norm (or a copy) into X.  For the planned r->B / H / W.
hipError_t head(hipStream_t s, const SwBase* r, const float* dev_x, int in_chans, float img_range, bool patch_norm)
{
    const long long HW = (long long)r->H * r->W, M = r->B * HW;
    GemmP p = gp_conv(dev_x, r->B, r->H, r->W, in_chans, r->wt + r->first_l.t, r->E, PP(r, r->first_l.b), r->XF, r->E);
    p.acs = HW; p.aps = 1;
    p.isub = r->mean; p.imul = img_range;
    hipError_t e = gemm(s, r, p);
    if (e) return e;
    if (patch_norm) return ln(s, r->XF, r->X, PP(r, r->pen_w), PP(r, r->pen_b), M, r->E);
    return hipMemcpyAsync(r->X, r->XF, sizeof(float) * M * r->E, hipMemcpyDeviceToDevice, s);
}

// x += fc2(gelu(fc1(norm2(x)))) on the M token rows of X; O is free, A takes the hidden rows
hipError_t mlp(hipStream_t s, const SwBase* r, float* X, float* O, long long M, long long n2w, long long n2b, const Lin& fc1, const Lin& fc2)
{
    const int E = r->E;
    hipError_t e = ln(s, X, O, PP(r, n2w), PP(r, n2b), M, E);
    if (e) return e;
    GemmP p = gp_tok(O, M, E, E, r->wt + fc1.t, r->hid, PP(r, fc1.b), r->A, r->hid);
    p.act = ACT_GELU;
    if ((e = gemm(s, r, p))) return e;
    p = gp_tok(r->A, M, r->hid, r->hid, r->wt + fc2.t, E, PP(r, fc2.b), X, E);
    p.res = X; p.rbs = 0; p.rps = E;
    return gemm(s, r, p);
}

// one Swin block's weights in the flat buffer (modules.py SwinTransformerBlock / WindowAttention / Mlp) and its shift
struct SBlk {
    long long n1w, n1b, table, n2w, n2b;
    Lin qkv, proj, fc1, fc2;
    int shift;
};

// SwinTransformerBlock (modules.py:299-350) on the token rows of X: x += proj(attn(norm1(x))); x += fc2(gelu(fc1(norm2(x)))).  O is free.
hipError_t swin_block(hipStream_t s, const SwBase* r, const SBlk& k, float* X, float* O, int B, int H, int W, int heads, float scale)
{
    const int E = r->E;
    const long long M = (long long)B * H * W;
    const float* wt = r->wt;
    hipError_t e;
    // norm1 into O (free until the attention writes it); a LayerNorm prologue inside the GEMM measured slower, DESIGN §12
    if ((e = ln(s, X, O, PP(r, k.n1w), PP(r, k.n1b), M, E))) return e;
    GemmP p = gp_tok(O, M, E, E, wt + k.qkv.t, 3 * E, PP(r, k.qkv.b), r->A, 3 * E);
    if ((e = gemm(s, r, p))) return e;
    if ((e = attention(s, r->A, O, r->params + k.table, B, H, W, E, heads, r->ws, k.shift, scale))) return e;
    p = gp_tok(O, M, E, E, wt + k.proj.t, E, PP(r, k.proj.b), X, E);
    p.res = X; p.rbs = 0; p.rps = E;
    if ((e = gemm(s, r, p))) return e;
    return mlp(s, r, X, O, M, k.n2w, k.n2b, k.fc1, k.fc2);
}

// conv_before_upsample + LeakyReLU(0.01), the PixelShuffle stages of Upsample, conv_last into NCHW x / img_range + mean.  With cH and
// cW (SW_GEMM_EXT) only the top-left cH x cW of the result is stored, as an image of that size.
hipError_t tail(hipStream_t s, const SwBase* r, const float* X, float* dev_y, int in_chans, int upscale, float img_range, int cH = 0, int cW = 0)
{
    const int B = r->B, nf = r->nfeat;
    GemmP p = gp_conv(X, B, r->H, r->W, r->E, r->wt + r->before.t, nf, PP(r, r->before.b), r->V, nf);
    p.act = ACT_LRELU; p.slope = 0.01f;
    hipError_t e = gemm(s, r, p);
    if (e) return e;
    const float* cur = r->V;
    int h = r->H, w = r->W;
    const int f = up_factor(upscale);
    for (size_t i = 0; i < r->ups.size(); ++i) {
        float* dst = (i % 2 == 0) ? r->U0 : r->U1;
        p = gp_conv(cur, B, h, w, nf, r->wt + r->ups[i].t, f * f * nf, PP(r, r->ups[i].b), dst, nf);
        p.omode = O_SHUFFLE; p.r = f; p.ybs = (long long)h * w * f * f * nf; p.yps = nf;
        if ((e = gemm(s, r, p))) return e;
        cur = dst; h *= f; w *= f;
    }
    p = gp_conv(cur, B, h, w, nf, r->wt + r->last.t, in_chans, PP(r, r->last.b), dev_y, 0);
    p.omode = O_NCHW; p.ybs = (long long)in_chans * h * w; p.omean = r->mean; p.orange = img_range;
    if (cW) { p.cH = cH; p.cW = cW; p.ybs = (long long)in_chans * cH * cW; }
    return gemm(s, r, p);
}

} // namespace

#endif /* XSD_SW_KERNELS_H */
