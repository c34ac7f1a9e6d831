// swinfir.hip -- the reference's SwinFIR super-resolution network (models/transformer/swinfir.py:120-441 with the Swin blocks of
// modules.py), FORWARD ONLY (eval mode: DropPath and Dropout are identities), in exact fp32.
//
// Every product is an fp32 FMA: the GEMMs and the attention on the fp32 matrix instruction v_mfma_f32_32x32x2_f32 (bitwise a
// k-ordered fmaf chain), the FFT butterflies on the vector ALUs.  The GEMMs' fmaf chains are 16 long, their sums over K are carried
// in double, as are the LayerNorm statistics.  No float atomics
// anywhere and every reduction has a fixed order: an image's output is bitwise independent of the batch it shares and of the run.
//
// Feature maps are TOKEN-MAJOR ([B][H*W][C], C contiguous): the Swin blocks' (B, L, C) layout, and the NHWC view of the same
// memory is what PatchUnEmbed / PatchEmbed (modules.py:423-500) turn into NCHW and back, so the convs of the SFB block, the head
// and the tail read and write it through their addressing; only the network input and output are NCHW.
//
// Kernels:
//   sw_gemm_kernel   C = A W (+ bias) on MFMA, 128 x 64 tile per workgroup.  A is either token rows (a Linear / 1x1 conv) or the
//                    implicit im2col of a 3x3 conv (zero pad 1; NCHW or token-major input, with
//                    the input affine (x - mean) * img_range of conv_first).  Epilogue: exact-erf GELU or LeakyReLU, residual add
//                    (may alias the output), and a token-major, PixelShuffle(r) or NCHW (x / img_range + mean) store.
//   sw_attn_kernel   one workgroup per (window, head): softmax(q scale k^T + table[index] (+ the -100 shift mask)) v, reading q, k,
//                    v from the qkv rows through the roll / window-partition addressing and writing the same way back.
//   sw_fft_kernel    one pass of the FourierUnit's 2-D transform (swinfir.py:14-61) over lines of one axis: R2C along W, complex
//                    along H (forward and inverse), C2R along W.  Mixed-radix Stockham in LDS with radices 4, 2, 3, 5, 7, 11, 13
//                    and twiddles from one table of the n-th roots of unity made in double.  The spectrum is stored as token rows
//                    [B][H][W/2+1][2 c + re/im]: the channel order of the reference's stack / permute / view, so the 1x1 conv
//                    over the spectrum is a plain token GEMM.
//   sw_ln_kernel     LayerNorm over the channels of each token (norm1 / norm2 in front of qkv / fc1, patch_embed.norm, the final
//                    norm), one wave per token, statistics in double.
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
// FFT
// ---------------------------------------------------------------------------------------------------------------
constexpr int FFT_MAXN = 4096;          // longest line: 2 buffers x n complex fill the 64 KiB of dynamic LDS
constexpr int FFT_MAXLINES = 16;
enum { F_R2C_ROWS = 0, F_COLS_FWD = 1, F_COLS_INV = 2, F_C2R_ROWS = 3 };

struct FftP {
    const float* in; float* out;
    int mode, n, lines;                 // transform length, lines (channels) per workgroup
    int H, W, Wk, C2;                   // image, W / 2 + 1 bins, complex channels
    const float2* tw;                   // tw[t] = exp(-2 pi i t / n), t < n
    int nrad, rad[16];
    float scale;
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <int R>
__device__ __forceinline__ void fft_pass(const float2* src, float2* dst, const FftP& P, int Ns, bool inv, int tid, int nthreads)
{
    const int n = P.n, nb = n / R, step = n / (Ns * R);
    for (int e = tid; e < P.lines * nb; e += nthreads) {
        const int l = e / nb, j = e - l * nb, k = j % Ns;
        const float2* s = src + l * n;
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = s[j + r * nb];
#pragma unroll
        for (int r = 1; r < R; ++r) {
            float2 w = P.tw[r * k * step];
            if (inv) w.y = -w.y;
            v[r] = cmul(v[r], w);
        }
        float2* d = dst + l * n + (j / Ns) * Ns * R + k;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            float2 acc = v[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                float2 w = P.tw[((r * q) % R) * nb];
                if (inv) w.y = -w.y;
                const float2 t = cmul(v[r], w);
                acc.x += t.x;
                acc.y += t.y;
            }
            d[q * Ns] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void sw_fft_kernel(const FftP P)
{
    extern __shared__ float2 fbuf[];
    const int tid = threadIdx.x, n = P.n, L = P.lines;
    float2* b0 = fbuf;
    float2* b1 = fbuf + L * n;
    const int line = blockIdx.x;               // rows: b H + y; columns: b Wk + kx
    const int c0 = blockIdx.y * L;
    const bool rows = P.mode == F_R2C_ROWS || P.mode == F_C2R_ROWS;
    const int b = rows ? line / P.H : line / P.Wk;
    const int y = rows ? line - b * P.H : 0, kx = rows ? 0 : line - b * P.Wk;
    const long long HW = (long long)P.H * P.W;
    const long long srow = 2ll * P.C2;         // floats per spectrum token
    for (int e = tid; e < L * n; e += 256) {
        const int t = e / L, l = e - t * L, c = c0 + l;
        float2 z = make_float2(0.f, 0.f);
        if (c < P.C2) {
            if (P.mode == F_R2C_ROWS) {
                z.x = P.in[((long long)b * HW + (long long)y * P.W + t) * P.C2 + c];
            } else if (P.mode == F_C2R_ROWS) {
                // bins 0 .. W/2 as stored, the rest their conjugates; the imaginary parts of DC and Nyquist do not enter (torch's C2R)
                const bool mir = t > n / 2;
                const int k = mir ? n - t : t;
                const float* s = P.in + ((long long)(b * P.H + y) * P.Wk + k) * srow + 2 * c;
                z = make_float2(s[0], (k == 0 || 2 * k == n) ? 0.f : (mir ? -s[1] : s[1]));
            } else {
                const float* s = P.in + ((long long)(b * P.H + t) * P.Wk + kx) * srow + 2 * c;
                z = make_float2(s[0], s[1]);
            }
        }
        b0[l * n + t] = z;
    }
    const bool inv = P.mode == F_COLS_INV || P.mode == F_C2R_ROWS;
    float2 *src = b0, *dst = b1;
    int Ns = 1;
    for (int st = 0; st < P.nrad; ++st) {
        __syncthreads();
        switch (P.rad[st]) {
        case 2: fft_pass<2>(src, dst, P, Ns, inv, tid, 256); break;
        case 3: fft_pass<3>(src, dst, P, Ns, inv, tid, 256); break;
        case 4: fft_pass<4>(src, dst, P, Ns, inv, tid, 256); break;
        case 5: fft_pass<5>(src, dst, P, Ns, inv, tid, 256); break;
        case 7: fft_pass<7>(src, dst, P, Ns, inv, tid, 256); break;
        case 11: fft_pass<11>(src, dst, P, Ns, inv, tid, 256); break;
        default: fft_pass<13>(src, dst, P, Ns, inv, tid, 256); break;
        }
        Ns *= P.rad[st];
        float2* t = src; src = dst; dst = t;
    }
    __syncthreads();
    if (P.mode == F_R2C_ROWS) {
        for (int e = tid; e < L * P.Wk; e += 256) {
            const int k = e / L, l = e - k * L, c = c0 + l;
            if (c >= P.C2) continue;
            const float2 z = src[l * n + k];
            float* d = P.out + ((long long)(b * P.H + y) * P.Wk + k) * srow + 2 * c;
            d[0] = z.x;
            d[1] = z.y;
        }
    } else if (P.mode == F_C2R_ROWS) {
        for (int e = tid; e < L * n; e += 256) {
            const int t = e / L, l = e - t * L, c = c0 + l;
            if (c >= P.C2) continue;
            P.out[((long long)b * HW + (long long)y * P.W + t) * P.C2 + c] += src[l * n + t].x * P.scale;   // x + fu(x)
        }
    } else {
        for (int e = tid; e < L * n; e += 256) {
            const int t = e / L, l = e - t * L, c = c0 + l;
            if (c >= P.C2) continue;
            const float2 z = src[l * n + t];
            float* d = P.out + ((long long)(b * P.H + t) * P.Wk + kx) * srow + 2 * c;
            d[0] = z.x * P.scale;
            d[1] = z.y * P.scale;
        }
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

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct Lin { long long w = -1, b = -1, t = -1; int cout = 0, cin = 0, taps = 1; };   // flat offsets of weight / bias, packed copy

struct SBlk {
    long long n1w, n1b, table, n2w, n2b;
    Lin qkv, proj, fc1, fc2;
    int shift;
};

struct Layer {
    std::vector<SBlk> blks;
    int heads;
    Lin s0, s2, c1, fu, c2, fus, conv1;      // SFB: S.body.0 / .2, F.conv1.0, F.fu.conv_layer, F.conv2, fusion; 1conv: conv
};

long long add(long long& off, long long n) { const long long o = off; off += n; return o; }

// the factorisation the FFT passes use: 4s first, then the primes <= 13; false if another prime divides n
bool radices(int n, std::vector<int>& out)
{
    out.clear();
    while (n % 4 == 0) { out.push_back(4); n /= 4; }
    for (int p : {2, 3, 5, 7, 11, 13})
        while (n % p == 0) { out.push_back(p); n /= p; }
    return n == 1 && out.size() <= 16;
}

} // namespace

struct xsd_swinfir {
    xsd_swinfir_config cfg;
    int E = 0, hid = 0, C2 = 0, ws = 0, nfeat = 64;
    bool clamped = false;
    long long nparams = 0, wt_floats = 0;
    long long first = 0, pen_w = -1, pen_b = -1, norm_w = 0, norm_b = 0;
    Lin first_l, after, before, last;
    std::vector<Lin> ups;
    std::vector<Layer> layers;
    std::vector<Lin*> lins;
    float* wt = nullptr;
    float* mean = nullptr;
    const float* params = nullptr;
    bool packed = false;
    int B = 0, H = 0, W = 0;
    char* ws_buf = nullptr;
    size_t ws_bytes = 0;
    float *XF = nullptr, *X = nullptr, *A = nullptr, *O = nullptr, *Y1 = nullptr, *S1 = nullptr, *S2 = nullptr, *V = nullptr,
          *U0 = nullptr, *U1 = nullptr, *R0 = nullptr;
    float2* tw = nullptr;             // roots of unity for H, then for W (device)
    int twH = 0, twW = 0;

    ~xsd_swinfir()
    {
        if (wt) hipFree(wt);
        if (mean) hipFree(mean);
        if (ws_buf) hipFree(ws_buf);
        if (tw) hipFree(tw);
    }
};

namespace {

void lin(Lin& l, long long& off, int cout, int cin, int taps, bool bias)
{
    l.cout = cout; l.cin = cin; l.taps = taps;
    l.w = add(off, (long long)cout * cin * taps);
    l.b = bias ? add(off, cout) : -1;
}

int up_stages(int s) { return s == 3 ? 1 : (int)std::lround(std::log2((double)s)); }
int up_factor(int s) { return s == 3 ? 3 : 2; }

// the reference's registration order (swinfir.py:267-401; modules.py RSTB / BasicLayer / SwinTransformerBlock / WindowAttention / Mlp)
void layout(xsd_swinfir* r)
{
    const auto& c = r->cfg;
    const int E = r->E, side = 2 * r->ws - 1;
    long long off = 0;
    lin(r->first_l, off, E, c.in_chans, 9, true);
    if (c.patch_norm) { r->pen_w = add(off, E); r->pen_b = add(off, E); }
    for (int li = 0; li < c.num_layers; ++li) {
        Layer L;
        L.heads = c.num_heads[li];
        for (int j = 0; j < c.depths[li]; ++j) {
            SBlk k{};
            k.shift = (j % 2 == 0 || r->clamped) ? 0 : c.window_size / 2;      // BasicLayer (modules.py:552)
            k.n1w = add(off, E); k.n1b = add(off, E);
            k.table = add(off, (long long)side * side * L.heads);
            lin(k.qkv, off, 3 * E, E, 1, c.qkv_bias != 0);
            lin(k.proj, off, E, E, 1, true);
            k.n2w = add(off, E); k.n2b = add(off, E);
            lin(k.fc1, off, r->hid, E, 1, true);
            lin(k.fc2, off, E, r->hid, 1, true);
            L.blks.push_back(k);
        }
        if (c.resi_connection == 0) {
            lin(L.s0, off, E, E, 9, true);
            lin(L.s2, off, E, E, 9, true);
            lin(L.c1, off, r->C2, E, 1, true);
            lin(L.fu, off, 2 * r->C2, 2 * r->C2, 1, true);
            lin(L.c2, off, E, r->C2, 1, true);
            lin(L.fus, off, E, 2 * E, 1, true);
        } else {
            lin(L.conv1, off, E, E, 9, true);
        }
        r->layers.push_back(L);
    }
    r->norm_w = add(off, E); r->norm_b = add(off, E);
    lin(r->after, off, E, E, 9, true);
    lin(r->before, off, r->nfeat, E, 9, true);
    const int f = up_factor(c.upscale);
    for (int s = 0; s < up_stages(c.upscale); ++s) {
        Lin u;
        lin(u, off, f * f * r->nfeat, r->nfeat, 9, true);
        r->ups.push_back(u);
    }
    lin(r->last, off, c.in_chans, r->nfeat, 9, true);
    r->nparams = off;
    r->lins.push_back(&r->first_l);
    for (auto& L : r->layers) {
        for (auto& k : L.blks)
            for (Lin* p : {&k.qkv, &k.proj, &k.fc1, &k.fc2}) r->lins.push_back(p);
        for (Lin* p : {&L.s0, &L.s2, &L.c1, &L.fu, &L.c2, &L.fus, &L.conv1})
            if (p->cout) r->lins.push_back(p);
    }
    for (Lin* p : {&r->after, &r->before}) r->lins.push_back(p);
    for (auto& u : r->ups) r->lins.push_back(&u);
    r->lins.push_back(&r->last);
    long long t = 0;
    for (Lin* p : r->lins) p->t = add(t, (long long)p->cout * p->cin * p->taps);
    r->wt_floats = t;
}

const float* PP(const xsd_swinfir* r, long long off) { return off < 0 ? nullptr : r->params + off; }

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

// qkv: token rows of 3 E (the qkv GEMM's output), out: token rows of E.  Both are passed by the caller: the forward's X / O roles
// change between layers (1conv swaps them), so nothing here may assume which workspace buffer holds what.
hipError_t attention(xsd_swinfir* r, hipStream_t s, const SBlk& k, int heads, const float* qkv, float* out)
{
    AttnP p{};
    p.qkv = qkv; p.o = out; p.table = r->params + k.table;
    p.H = r->H; p.W = r->W; p.C = r->E; p.heads = heads; p.hd = r->E / heads; p.ws = r->ws; p.shift = k.shift;
    p.nwx = r->W / r->ws; p.nw = (r->H / r->ws) * p.nwx;
    p.scale = r->cfg.qk_scale > 0 ? (float)r->cfg.qk_scale : (float)std::pow((double)p.hd, -0.5);    // `qk_scale or head_dim ** -0.5`
    dim3 grid((unsigned)(r->B * p.nw), (unsigned)heads);
    const int nt = (r->ws * r->ws + 31) / 32;
    switch (nt) {
#define SW_ATT(T) case T: hipLaunchKernelGGL(sw_attn_kernel<T>, grid, dim3(64 * T), 0, s, p); break;
    SW_ATT(1) SW_ATT(2) SW_ATT(3) SW_ATT(4) SW_ATT(5) SW_ATT(6) SW_ATT(7) SW_ATT(8)
#undef SW_ATT
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// what one FFT pass needs to know: the shape and the twiddle table (H roots, then W roots); a view, it owns nothing
struct FftShape { int B, H, W, C2; const float2* tw; };

hipError_t fft(const FftShape& r, hipStream_t s, int mode, const float* in, float* out)
{
    FftP p{};
    p.in = in; p.out = out; p.mode = mode;
    const bool rows = mode == F_R2C_ROWS || mode == F_C2R_ROWS;
    p.n = rows ? r.W : r.H;
    p.H = r.H; p.W = r.W; p.Wk = r.W / 2 + 1; p.C2 = r.C2;
    p.tw = rows ? r.tw + r.H : r.tw;
    std::vector<int> rad;
    radices(p.n, rad);
    p.nrad = (int)rad.size();
    for (int i = 0; i < p.nrad; ++i) p.rad[i] = rad[i];
    p.lines = std::max(1, std::min(FFT_MAXLINES, FFT_MAXN / p.n));
    // the ortho scale 1 / sqrt(H W) once, after the second axis of each direction
    p.scale = (mode == F_COLS_FWD || mode == F_C2R_ROWS) ? (float)(1.0 / std::sqrt((double)r.H * r.W)) : 1.f;
    dim3 grid((unsigned)(r.B * (rows ? r.H : p.Wk)), (unsigned)((r.C2 + p.lines - 1) / p.lines));
    hipLaunchKernelGGL(sw_fft_kernel, grid, dim3(256), (size_t)2 * p.lines * p.n * sizeof(float2), s, p);
    return hipGetLastError();
}

hipError_t ln(hipStream_t s, const float* x, float* y, const float* w, const float* b, long long M, int C)
{
    hipLaunchKernelGGL(sw_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, y, w, b, M, C);
    return hipGetLastError();
}

// workspace of one (B, H, W) in floats; with `assign` set, also the pointers into r->ws_buf
long long plan_ws(xsd_swinfir* r, int B, int H, int W, bool assign)
{
    const long long M = (long long)B * H * W, E = r->E, Ms = (long long)B * H * (W / 2 + 1);
    const long long up = (long long)r->cfg.upscale * r->cfg.upscale;
    const long long sizes[11] = {M * E, M * E, M * std::max({3 * E, (long long)r->hid, 2 * E}), M * E, M * r->C2, Ms * 2 * r->C2,
                                 Ms * 2 * r->C2, M * r->nfeat, M * up * r->nfeat, M * up * r->nfeat, M * E};
    float** ptrs[11] = {&r->XF, &r->X, &r->A, &r->O, &r->Y1, &r->S1, &r->S2, &r->V, &r->U0, &r->U1, &r->R0};
    long long off = 0;
    for (int i = 0; i < 11; ++i) {
        if (assign) *ptrs[i] = (float*)r->ws_buf + off;
        off += (std::max(sizes[i], 1ll) + 63) / 64 * 64;        // 256-B aligned
    }
    return off;
}

int set_twiddles(xsd_swinfir* r, int H, int W)
{
    if (r->twH == H && r->twW == W) return XSD_OK;
    const double pi = std::acos(-1.0);
    std::vector<float2> t((size_t)H + W);
    for (int i = 0; i < H; ++i) t[i] = make_float2((float)std::cos(-2.0 * pi * i / H), (float)std::sin(-2.0 * pi * i / H));
    for (int i = 0; i < W; ++i) t[H + i] = make_float2((float)std::cos(-2.0 * pi * i / W), (float)std::sin(-2.0 * pi * i / W));
    if (r->tw) { hipDeviceSynchronize(); hipFree(r->tw); r->tw = nullptr; r->twH = r->twW = 0; }
    if (hipMalloc((void**)&r->tw, sizeof(float2) * t.size()) != hipSuccess) {
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "SwinFIR: twiddle table allocation failed");
    }
    if (hipMemcpy(r->tw, t.data(), sizeof(float2) * t.size(), hipMemcpyHostToDevice) != hipSuccess)
        return rfail(XSD_ERR_HIP, "SwinFIR: twiddle table upload failed");
    r->twH = H; r->twW = W;
    return XSD_OK;
}

const char* upsampler_name(int u)
{
    switch (u) { case 0: return "pixelshuffle"; case 1: return "pixelshuffledirect"; case 2: return "nearest+conv"; default: return "\"\" (none)"; }
}

const char* resi_name(int u)
{
    switch (u) { case 0: return "SFB"; case 1: return "1conv"; case 2: return "HSFB"; default: return "identity"; }
}

} // namespace

extern "C" {

int xsd_swinfir_fft_supported(int n)
{
    std::vector<int> rad;
    return n >= 1 && n <= FFT_MAXN && radices(n, rad) ? 1 : 0;
}

int xsd_swinfir_create(const xsd_swinfir_config* cfg, xsd_swinfir** out)
{
    if (!cfg || !out) return rfail(XSD_ERR_ARG, "null argument");
    *out = nullptr;
    const auto& c = *cfg;
    if (c.ape) return rfail(XSD_ERR_ARG, "SwinFIR: ape=True (absolute position embedding) is not supported by the MI355X engine");
    if (c.upsampler != 0)
        return rfail(XSD_ERR_ARG, "SwinFIR: upsampler %s is not supported by the MI355X engine (only \"pixelshuffle\")", upsampler_name(c.upsampler));
    if (c.resi_connection != 0 && c.resi_connection != 1)
        return rfail(XSD_ERR_ARG, "SwinFIR: resi_connection %s is not supported by the MI355X engine (only \"SFB\" and \"1conv\")",
                     resi_name(c.resi_connection));
    if (c.in_chans < 1 || c.in_chans > 64) return rfail(XSD_ERR_ARG, "SwinFIR: in_chans must be in [1, 64] (got %d)", c.in_chans);
    if (c.embed_dim < 2 || c.embed_dim > 4096) return rfail(XSD_ERR_ARG, "SwinFIR: embed_dim must be in [2, 4096] (got %d)", c.embed_dim);
    if (c.num_layers < 0 || c.num_layers > 16) return rfail(XSD_ERR_ARG, "SwinFIR: at most 16 layers (got %d)", c.num_layers);
    if (c.upscale != 2 && c.upscale != 3 && c.upscale != 4 && c.upscale != 8)
        return rfail(XSD_ERR_ARG, "SwinFIR: upscale %d is not supported (2^n and 3, modules.py Upsample)", c.upscale);
    if (!(c.img_range > 0)) return rfail(XSD_ERR_ARG, "SwinFIR: img_range must be positive");
    if (!(c.qk_scale >= 0))
        return rfail(XSD_ERR_ARG, "SwinFIR: qk_scale %g is not supported (None / 0 for head_dim^-0.5, or a positive scale)", c.qk_scale);
    if (!(c.mlp_ratio > 0) || (int)(c.embed_dim * c.mlp_ratio) < 1 || c.embed_dim * c.mlp_ratio > 65536)
        return rfail(XSD_ERR_ARG, "SwinFIR: mlp_ratio %g gives no usable hidden width", c.mlp_ratio);
    if (c.img_size[0] < 1 || c.img_size[1] < 1 || c.patch_size[0] < 1 || c.patch_size[1] < 1 || c.window_size < 1)
        return rfail(XSD_ERR_ARG, "SwinFIR: img_size, patch_size and window_size must be positive");
    const int res = std::min(c.img_size[0] / c.patch_size[0], c.img_size[1] / c.patch_size[1]);
    const bool clamped = res <= c.window_size;                      // SwinTransformerBlock.__init__ (modules.py:236-239): no shift then
    const int ws = clamped ? res : c.window_size;
    if (ws < 1) return rfail(XSD_ERR_ARG, "SwinFIR: img_size // patch_size is 0");
    if (ws > 16) return rfail(XSD_ERR_ARG, "SwinFIR: an effective window of %d exceeds the engine's 16 (256 tokens per window)", ws);
    for (int l = 0; l < c.num_layers; ++l) {
        if (c.depths[l] < 0 || c.depths[l] > 64) return rfail(XSD_ERR_ARG, "SwinFIR: depths[%d] must be in [0, 64]", l);
        const int h = c.num_heads[l];
        if (h < 1 || c.embed_dim % h) return rfail(XSD_ERR_ARG, "SwinFIR: num_heads[%d] = %d does not divide embed_dim %d", l, h, c.embed_dim);
        if (c.embed_dim / h > 32) return rfail(XSD_ERR_ARG, "SwinFIR: head dim %d at layer %d; the engine takes at most 32", c.embed_dim / h, l);
    }
    if (c.resi_connection == 0 && c.embed_dim < 2) return rfail(XSD_ERR_ARG, "SwinFIR: SFB needs embed_dim >= 2");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return rfail(XSD_ERR_HIP, "no HIP device available");
    xsd_swinfir* r = new xsd_swinfir();
    r->cfg = c;
    r->E = c.embed_dim;
    r->hid = (int)(c.embed_dim * c.mlp_ratio);
    r->C2 = c.embed_dim / 2;
    r->ws = ws;
    r->clamped = clamped;
    layout(r);
    std::vector<float> mean(c.in_chans, 0.f);
    if (c.in_chans == 3) { mean[0] = 0.3014f; mean[1] = 0.3152f; mean[2] = 0.3094f; }   // swinfir.py:319-323
    if (hipMalloc((void**)&r->wt, sizeof(float) * std::max(1ll, r->wt_floats)) != hipSuccess ||
        hipMalloc((void**)&r->mean, sizeof(float) * c.in_chans) != hipSuccess ||
        hipMemcpy(r->mean, mean.data(), sizeof(float) * c.in_chans, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        delete r;
        return rfail(XSD_ERR_NOMEM, "SwinFIR: packed-weight allocation failed");
    }
    *out = r;
    return XSD_OK;
}

void xsd_swinfir_destroy(xsd_swinfir* r) { delete r; }

int64_t xsd_swinfir_param_count(const xsd_swinfir* r) { return r ? r->nparams : -1; }

int xsd_swinfir_pack_weights(xsd_swinfir* r, const float* dev_params, void* stream)
{
    if (!r || !dev_params) return rfail(XSD_ERR_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    r->params = dev_params;
    for (const Lin* p : r->lins) {
        const long long n = (long long)p->cout * p->cin * p->taps;
        hipLaunchKernelGGL(sw_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dev_params + p->w, r->wt + p->t, p->cout, p->cin, p->taps);
        hipError_t e = hipGetLastError();
        if (e) return rfail(XSD_ERR_HIP, "SwinFIR weight packing: %s", hipGetErrorString(e));
    }
    r->packed = true;
    return XSD_OK;
}

int xsd_swinfir_forward(xsd_swinfir* r, const float* dev_x, float* dev_y, int B, int H, int W, void* stream)
{
    if (!r || !dev_x || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "bad shape %dx%dx%d", B, H, W);
    if (H % r->ws || W % r->ws)
        return rfail(XSD_ERR_ARG, "SwinFIR: H and W must be multiples of the window size %d (window_partition); got %d x %d", r->ws, H, W);
    if (r->cfg.resi_connection == 0)
        for (int n : {H, W})
            if (!xsd_swinfir_fft_supported(n))
                return rfail(XSD_ERR_ARG, "SwinFIR: FFT size %d is not supported (the FourierUnit needs H and W of at most %d whose prime factors are all "
                             "<= 13); got %d x %d", n, FFT_MAXN, H, W);
    const long long up = r->cfg.upscale;
    if ((long long)H * W * up * up > (1ll << 28)) return rfail(XSD_ERR_ARG, "SwinFIR: image of %d x %d pixels is too large", H, W);
    if (!r->packed) return rfail(XSD_ERR_STATE, "xsd_swinfir_pack_weights must be called before xsd_swinfir_forward");
    hipStream_t s = (hipStream_t)stream;
    if (r->B != B || r->H != H || r->W != W) {
        const size_t need = sizeof(float) * (size_t)plan_ws(r, B, H, W, false) + 256;
        if (need > r->ws_bytes) {
            // refused BEFORE the held workspace is given up or anything is enqueued: the engine stays usable at its last shape
            const double gb = 1.0 / (1024.0 * 1024.0 * 1024.0);
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b + r->ws_bytes)
                return rfail(XSD_ERR_NOMEM, "SwinFIR: a workspace of %.1f GiB for %d x %d x %d tiles does not fit this device (%.1f GiB free + %.1f GiB held "
                             "by this engine of %.1f GiB); use a smaller batch per call", need * gb, B, H, W, free_b * gb, r->ws_bytes * gb, total_b * gb);
            if (r->ws_buf) { hipDeviceSynchronize(); hipFree(r->ws_buf); r->ws_buf = nullptr; r->ws_bytes = 0; r->B = r->H = r->W = 0; }
            hipError_t err = hipMalloc((void**)&r->ws_buf, need);
            if (err != hipSuccess) {
                (void)hipGetLastError();
                return rfail(XSD_ERR_NOMEM, "SwinFIR: workspace hipMalloc(%.1f GiB for %d x %d x %d tiles) failed: %s", need * gb, B, H, W, hipGetErrorString(err));
            }
            r->ws_bytes = need;
        }
        int rc = set_twiddles(r, H, W);
        if (rc) return rc;
        plan_ws(r, B, H, W, true);
        r->B = B; r->H = H; r->W = W;
    }
    const auto& c = r->cfg;
    const int E = r->E, C2 = r->C2, nf = r->nfeat;
    const long long HW = (long long)H * W, M = B * HW, Ms = (long long)B * H * (W / 2 + 1);
    float* X = r->X;
    float* O = r->O;
    float* const XF = r->XF;
    const FftShape fs{B, H, W, C2, r->tw};
    const float* wt = r->wt;
    hipError_t e = hipSuccess;
#define SW(x) do { if ((e = (x)) != hipSuccess) return rfail(XSD_ERR_HIP, "SwinFIR forward: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__); } while (0)
    {   // conv_first over (x - mean) * img_range (swinfir.py:425-430), NCHW in
        GemmP p = gp_conv(dev_x, B, H, W, c.in_chans, wt + r->first_l.t, E, PP(r, r->first_l.b), XF, E);
        p.acs = HW; p.aps = 1;
        p.isub = r->mean; p.imul = (float)c.img_range;
        SW(gemm(s, p));
    }
    if (c.patch_norm) SW(ln(s, XF, X, PP(r, r->pen_w), PP(r, r->pen_b), M, E));         // patch_embed (modules.py:455-461)
    else SW(hipMemcpyAsync(X, XF, sizeof(float) * M * E, hipMemcpyDeviceToDevice, s));
    for (const Layer& L : r->layers) {
        // the RSTB's input: its `+ x` (swinfir.py:214-216) adds it after the blocks and the conv
        SW(hipMemcpyAsync(r->R0, X, sizeof(float) * M * E, hipMemcpyDeviceToDevice, s));
        for (const SBlk& k : L.blks) {
            // SwinTransformerBlock (modules.py:299-350): x += proj(attn(norm1(x))); x += fc2(gelu(fc1(norm2(x))))
            // norm1 into O (free until the attention writes it); a LayerNorm prologue inside the GEMM measured slower, DESIGN §12
            SW(ln(s, X, O, PP(r, k.n1w), PP(r, k.n1b), M, E));
            GemmP p = gp_tok(O, M, E, E, wt + k.qkv.t, 3 * E, PP(r, k.qkv.b), r->A, 3 * E);
            SW(gemm(s, p));
            SW(attention(r, s, k, L.heads, r->A, O));
            p = gp_tok(O, M, E, E, wt + k.proj.t, E, PP(r, k.proj.b), X, E);
            p.res = X; p.rbs = 0; p.rps = E;
            SW(gemm(s, p));
            SW(ln(s, X, O, PP(r, k.n2w), PP(r, k.n2b), M, E));                                  // norm2 into O
            p = gp_tok(O, M, E, E, wt + k.fc1.t, r->hid, PP(r, k.fc1.b), r->A, r->hid);
            p.act = ACT_GELU;
            SW(gemm(s, p));
            p = gp_tok(r->A, M, r->hid, r->hid, wt + k.fc2.t, E, PP(r, k.fc2.b), X, E);
            p.res = X; p.rbs = 0; p.rps = E;
            SW(gemm(s, p));
        }
        if (c.resi_connection == 0) {
            // RSTB tail x = SFB(x) + RSTB input (swinfir.py:103-117, :214-216); CAT = [S | F] as the row halves of the A buffer
            float* CAT = r->A;
            GemmP p = gp_conv(X, B, H, W, E, wt + L.s0.t, E, PP(r, L.s0.b), O, E);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, p));
            p = gp_conv(O, B, H, W, E, wt + L.s2.t, E, PP(r, L.s2.b), CAT, 2 * E);
            p.res = X; p.rbs = HW * E; p.rps = E;
            SW(gemm(s, p));
            p = gp_tok(X, M, E, E, wt + L.c1.t, C2, PP(r, L.c1.b), r->Y1, C2);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, p));
            SW(fft(fs, s, F_R2C_ROWS, r->Y1, r->S1));
            SW(fft(fs, s, F_COLS_FWD, r->S1, r->S1));
            p = gp_tok(r->S1, Ms, 2 * C2, 2 * C2, wt + L.fu.t, 2 * C2, PP(r, L.fu.b), r->S2, 2 * C2);
            p.act = ACT_LRELU; p.slope = 0.2f;
            SW(gemm(s, p));
            SW(fft(fs, s, F_COLS_INV, r->S2, r->S2));
            SW(fft(fs, s, F_C2R_ROWS, r->S2, r->Y1));                                             // Y1 = x + fu(x)
            p = gp_tok(r->Y1, M, C2, C2, wt + L.c2.t, E, PP(r, L.c2.b), CAT + E, 2 * E);
            SW(gemm(s, p));
            p = gp_tok(CAT, M, 2 * E, 2 * E, wt + L.fus.t, E, PP(r, L.fus.b), X, E);
            p.res = r->R0; p.rbs = 0; p.rps = E;
            SW(gemm(s, p));
        } else {
            GemmP p = gp_conv(X, B, H, W, E, wt + L.conv1.t, E, PP(r, L.conv1.b), O, E);
            p.res = r->R0; p.rbs = HW * E; p.rps = E;
            SW(gemm(s, p));
            std::swap(X, O);
        }
    }
    // norm, conv_after_body + conv_first's output, conv_before_upsample + LeakyReLU(0.01), Upsample, conv_last (swinfir.py:430-433)
    SW(ln(s, X, O, PP(r, r->norm_w), PP(r, r->norm_b), M, E));
    {
        GemmP p = gp_conv(O, B, H, W, E, wt + r->after.t, E, PP(r, r->after.b), X, E);
        p.res = XF; p.rbs = HW * E; p.rps = E;
        SW(gemm(s, p));
        p = gp_conv(X, B, H, W, E, wt + r->before.t, nf, PP(r, r->before.b), r->V, nf);
        p.act = ACT_LRELU; p.slope = 0.01f;
        SW(gemm(s, p));
    }
    const float* cur = r->V;
    int h = H, w = W;
    const int f = up_factor(c.upscale);
    for (size_t i = 0; i < r->ups.size(); ++i) {
        float* dst = (i % 2 == 0) ? r->U0 : r->U1;
        GemmP p = gp_conv(cur, B, h, w, nf, wt + r->ups[i].t, f * f * nf, PP(r, r->ups[i].b), dst, nf);
        p.omode = O_SHUFFLE; p.r = f; p.ybs = (long long)h * w * f * f * nf; p.yps = nf;
        SW(gemm(s, p));
        cur = dst; h *= f; w *= f;
    }
    {
        GemmP p = gp_conv(cur, B, h, w, nf, wt + r->last.t, c.in_chans, PP(r, r->last.b), dev_y, 0);
        p.omode = O_NCHW; p.ybs = (long long)c.in_chans * h * w; p.omean = r->mean; p.orange = (float)c.img_range;
        SW(gemm(s, p));
    }
#undef SW
    return XSD_OK;
}

// the FourierUnit's transform pair on its own (tests): x [B][H][W][C2] real (token-major) -> spec [B][H][W/2+1][2 C2] = rfftn(ortho),
// and, with inverse set, spec -> x += irfftn(spec, s=(H, W), ortho).  Needs an engine for the twiddle table; takes no weights.
int xsd_swinfir_test_fft(xsd_swinfir* r, float* dev_x, float* dev_spec, int B, int H, int W, int C2, int inverse, void* stream)
{
    if (!r || !dev_x || !dev_spec) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || C2 < 1) return rfail(XSD_ERR_ARG, "bad shape");
    for (int n : {H, W})
        if (!xsd_swinfir_fft_supported(n))
            return rfail(XSD_ERR_ARG, "SwinFIR: FFT size %d is not supported (at most %d, prime factors <= 13)", n, FFT_MAXN);
    hipStream_t s = (hipStream_t)stream;
    if (r->twH != H || r->twW != W) {
        hipStreamSynchronize(s);
        int rc = set_twiddles(r, H, W);
        if (rc) return rc;
        r->B = r->H = r->W = 0;          // the workspace plan no longer matches the twiddles: re-plan at the next forward
    }
    const FftShape fs{B, H, W, C2, r->tw};
    hipError_t e = inverse ? fft(fs, s, F_COLS_INV, dev_spec, dev_spec) : fft(fs, s, F_R2C_ROWS, dev_x, dev_spec);
    if (!e) e = inverse ? fft(fs, s, F_C2R_ROWS, dev_spec, dev_x) : fft(fs, s, F_COLS_FWD, dev_spec, dev_spec);
    if (e) return rfail(XSD_ERR_HIP, "SwinFIR FFT test: %s", hipGetErrorString(e));
    return XSD_OK;
}

} // extern "C"
