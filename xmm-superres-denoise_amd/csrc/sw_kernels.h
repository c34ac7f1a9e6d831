// sw_kernels.h -- HAT's copy of the exact-fp32 kernels it shares with SwinFIR: the MFMA GEMM with its conv3x3 mode and epilogues, the
// (shifted-)window attention, the LayerNorm, the weight packing, and their launch helpers, taken unchanged from swinfir.hip.  Only
// hat.hip includes this file: swinfir.hip keeps its own definitions, so that SwinFIR's code does not change with HAT's arrival.  A change
// to one of these kernels belongs in both places (or in a move of swinfir.hip onto this header, checked bitwise on SwinFIR's goldens).
// Everything is in an anonymous namespace.
#ifndef XSD_SW_KERNELS_H
#define XSD_SW_KERNELS_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/xsd.h"

namespace xsd {
int set_last_error(int code, const std::string& msg);     // xsd_engine.hip: the thread-local message of xsd_last_error()
}

namespace {

int rfail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return xsd::set_last_error(code, buf);
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------
constexpr int GM = 128;      // rows (tokens / pixels) per workgroup: wave w owns rows [32 w, 32 w + 32)
constexpr int GN = 64;       // output columns per workgroup: two 32 x 32 accumulators per wave
constexpr int GK = 16;       // K per LDS round
constexpr int GAP = GM + 4;  // LDS row pitch of the A tile

enum { A_TOK = 0, A_CONV3 = 1 };
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_LRELU = 2 };
enum { O_TOK = 0, O_SHUFFLE = 1, O_NCHW = 2 };

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
};

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
                    v = P.a[rbase[i] + (long long)ci * P.acs + ((long long)yy * P.W + xx) * P.aps];
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

    // each K round is a 16-term fmaf chain on the MFMA from zero; the rounds are summed in double (a fixed order)
    double d0[16], d1[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) { d0[v] = 0.0; d1[v] = 0.0; }
    const int i32 = lane & 31, h2 = lane >> 5;
    load(0);
    for (int k0 = 0; k0 < P.K; k0 += GK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) As[kl][(tid >> 4) + 16 * i] = av[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[(tid >> 6) + 4 * i][tid & 63] = bv[i];
        __syncthreads();
        if (k0 + GK < P.K) load(k0 + GK);
        f32x16 acc0, acc1;
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
#pragma unroll
        for (int s = 0; s < GK / 2; ++s) {
            const float a = As[2 * s + h2][32 * wave + i32];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[2 * s + h2][i32], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[2 * s + h2][32 + i32], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) { d0[v] += (double)acc0[v]; d1[v] += (double)acc1[v]; }
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
            float x = (float)(c ? d1[v] : d0[v]) + bn;
            if (P.act == ACT_GELU) x = 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
            else if (P.act == ACT_LRELU) x = x >= 0.f ? x : x * P.slope;
            const long long b = m / P.HW, p = m - b * P.HW;
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

struct Lin { long long w = -1, b = -1, t = -1; int cout = 0, cin = 0, taps = 1; };   // flat offsets of weight / bias, packed copy

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

hipError_t gemm(hipStream_t s, const GemmP& p)
{
    const long long M = (long long)p.B * p.HW;
    dim3 grid((unsigned)((M + GM - 1) / GM), (unsigned)((p.N + GN - 1) / GN));
    hipLaunchKernelGGL(sw_gemm_kernel, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t ln(hipStream_t s, const float* x, float* y, const float* w, const float* b, long long M, int C)
{
    hipLaunchKernelGGL(sw_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, y, w, b, M, C);
    return hipGetLastError();
}

} // namespace

#endif /* XSD_SW_KERNELS_H */
