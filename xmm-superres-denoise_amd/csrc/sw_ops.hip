// sw_ops.hip -- the four Swin operations of sw_kernels.h as stand-alone differentiable ops (include/xsd.h, "differentiable Swin ops"):
// linear, conv3x3, layer_norm and window_attention, one forward and one backward entry each, for torch.autograd.Functions that compose a
// trainable network in Python (xmm_superres_denoise/ops.py, models/modules/swinir_train.py).
//
// The forwards of layer_norm and window_attention are sw_kernels.h's kernels with the arguments of the xsd_sw_test_* hooks (this file
// compiles its own instance of them, as swinfir.hip, hat.hip and swinir.hip do).  linear and conv3x3 run ops_conv_kernel, forward and
// input gradient: sw_gemm_kernel's tile and (implicit im2col) staging, but every product joins a double sum on the vector ALUs and the
// bias joins it too, so each result is the exact one rounded once.  Why not sw_gemm_kernel: torch's fp32 conv of small sizes accumulates
// in double, and a network's parameter gradients are held to twice torch's fp32 error tensor by tensor; with fp32 chains of 16 the
// 12-element gradients of a tiny network landed at 2 to 3 times it.
// The backwards:
//   linear / conv3x3   dz = dy act'(z) (ops_act_bwd_kernel, the derivative in double); da = dz W (the stored weight is the [K][N]
//                      matrix the kernel reads); dx = ops_conv_kernel(dz, W flipped and transposed); dW and db on
//                      ops_wgrad_kernel (rows = cout, K = a chunk of tokens, the bias gradient as one more column against a
//                      constant 1, every product into a double sum) into one partial per chunk, summed in ascending chunk order by
//                      ops_wgrad_reduce_kernel.
//   layer_norm         ops_ln_bwd_kernel (one wave per token, everything in double) + per-chunk partials of dgamma / dbeta.
//   window_attention   ops_attn_bwd_kernel, one workgroup per (window, head): the probabilities are recomputed from qkv, 8 query rows
//                      of P and dS at a time live in LDS, dq leaves per row block, dk / dv / the bias-table bins are carried in
//                      registers across the row blocks (each thread owns its (key, channel) pairs and its bins and walks the query
//                      rows in ascending order), one table partial per (window, head), summed in a fixed order afterwards.
// Every product of the backward is an exact fp32 product added in double; no float atomics;
// every reduction has a fixed order; nothing here allocates or synchronises: scratch is the caller's.
#include "sw_kernels.h"

namespace {

constexpr long long OPS_MAX_ROWS = 1ll << 28;
constexpr int OPS_MAX_CHUNKS = 4096;
constexpr int LN_ROWS = 128;         // rows per dgamma / dbeta partial

// sw_kernels.h declares the GEMM "in the engine's math mode" for its block helpers; no engine here, and fp32 only
hipError_t gemm(hipStream_t s, const SwBase*, const GemmP& p) { return gemm(s, p); }

long long al256(long long bytes) { return (bytes + 255) & ~255ll; }

// ---------------------------------------------------------------------------------------------------------------
// activations
// ---------------------------------------------------------------------------------------------------------------
// y = act(z): the expressions of sw_gemm_kernel's epilogue, so that act(z) of a stored pre-activation is the fused result bit for bit
__global__ __launch_bounds__(256) void ops_act_kernel(const float* z, float* y, long long n, int act, float slope)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float x = z[i];
    if (act == ACT_GELU) x = 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
    else if (act == ACT_LRELU) x = x >= 0.f ? x : x * slope;
    y[i] = x;
}

// dz = dy act'(z), the derivative in double: GELU' = Phi(z) + z phi(z)
__global__ __launch_bounds__(256) void ops_act_bwd_kernel(const float* dy, const float* z, float* dz, long long n, int act, float slope)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)z[i];
    double d;
    if (act == ACT_GELU) d = 0.5 * (1.0 + erf(x * 0.70710678118654752440)) + x * exp(-0.5 * x * x) * 0.39894228040143267794;
    else d = z[i] >= 0.f ? 1.0 : (double)slope;
    dz[i] = (float)((double)dy[i] * d);
}

// ---------------------------------------------------------------------------------------------------------------
// the 128 x 64 x 16 tile on the vector ALUs: acc[i][j] += As[k][8 ty + i] * Bs[k][4 tx + j], each exact fp32 product added in double
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_fma(const float (*As)[GAP], const float (*Bs)[GN], int ty, int tx, double (&acc)[8][4])
{
#pragma unroll 4
    for (int k = 0; k < GK; ++k) {
        double a[8], b[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (double)As[k][8 * ty + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = (double)Bs[k][4 * tx + j];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// a Linear over token rows, or a 3x3 conv (zero pad 1) over token-major images, with the whole sum over K in double:
// y = act(x * w + bias), one rounding to fp32.  Forward and, with the transposed (and flipped) weight, the input gradient.
// ---------------------------------------------------------------------------------------------------------------
struct ConvP {
    const float* x; int B, H, W, cin;    // [B][H][W][cin]
    int lin;                             // 1: no taps, a Linear over the B H W token rows (K = cin)
    const float* w; int N;               // [K][N]; conv: K = 9 cin, k = tap cin + ci
    const float* bias;                   // [N] or null
    int act; float slope;
    float* y;                            // [B][H][W][N]
};

__global__ __launch_bounds__(256) void ops_conv_kernel(const ConvP P)
{
    __shared__ __attribute__((aligned(16))) float As[GK][GAP];
    __shared__ __attribute__((aligned(16))) float Bs[GK][GN];
    const int tid = threadIdx.x, K = P.lin ? P.cin : 9 * P.cin;
    const long long HW = (long long)P.H * P.W, M = P.B * HW;
    const long long m0 = (long long)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;
    // the rows this thread stages: (tid >> 4) + 16 i, at k = k0 + (tid & 15)
    const int kl = tid & 15;
    long long rbase[8];
    int ry[8], rx[8];
    bool rok[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long long m = m0 + (tid >> 4) + 16 * i;
        rok[i] = m < M;
        const long long b = rok[i] ? m / HW : 0, p = rok[i] ? m - b * HW : 0;
        rbase[i] = P.lin ? m : b * HW;
        ry[i] = (int)(p / P.W);
        rx[i] = (int)(p - (long long)ry[i] * P.W);
    }
    float av[8], bv[4];
    auto load = [&](int k0) {
        const int k = k0 + kl;
        const bool kok = k < K;
        if (P.lin) {
#pragma unroll
            for (int i = 0; i < 8; ++i) av[i] = (rok[i] && kok) ? P.x[rbase[i] * P.cin + k] : 0.f;
        } else {
            const int tap = kok ? k / P.cin : 0, ci = kok ? k - tap * P.cin : 0;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int yy = ry[i] + dy, xx = rx[i] + dx;
                av[i] = (rok[i] && kok && yy >= 0 && yy < P.H && xx >= 0 && xx < P.W) ? P.x[(rbase[i] + (long long)yy * P.W + xx) * P.cin + ci] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = k0 + (tid >> 6) + 4 * i, n = n0 + (tid & 63);
            bv[i] = (kk < K && n < P.N) ? P.w[(long long)kk * P.N + n] : 0.f;
        }
    };
    double acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    const int ty = tid >> 4, tx = tid & 15;
    load(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) As[kl][(tid >> 4) + 16 * i] = av[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[(tid >> 6) + 4 * i][tid & 63] = bv[i];
        __syncthreads();
        if (k0 + GK < K) load(k0 + GK);
        tile_fma(As, Bs, ty, tx, acc);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 4 * tx + j;
        if (n >= P.N) continue;
        const double bn = P.bias ? (double)P.bias[n] : 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long long m = m0 + 8 * ty + i;
            if (m >= M) continue;
            float x = (float)(acc[i][j] + bn);
            if (P.act == ACT_GELU) x = 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
            else if (P.act == ACT_LRELU) x = x >= 0.f ? x : x * P.slope;
            P.y[m * P.N + n] = x;
        }
    }
}

// lin: a Linear over M = B H W rows (pass B = 1, H = 1, W = M <= 2^28)
hipError_t conv(hipStream_t s, const float* x, int B, int H, int W, int cin, const float* w, int N, const float* bias, int act, float slope, float* y,
                int lin = 0)
{
    ConvP p{x, B, H, W, cin, lin, w, N, bias, act, slope, y};
    const long long M = (long long)B * H * W;
    hipLaunchKernelGGL(ops_conv_kernel, dim3((unsigned)((M + GM - 1) / GM), (unsigned)((N + GN - 1) / GN)), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient: part[c][n][k] = sum over the tokens t of chunk c of dz[t][n] * A[t][k]
// ---------------------------------------------------------------------------------------------------------------
struct WgP {
    const float* dz; int N;          // [M][N]
    const float* a;                  // linear: [M][Kw]; conv: [B][H][W][cin] token-major
    int conv, H, W, cin, Kw, Kp;     // Kw = taps cin (k = tap cin + ci), Kp = Kw + 1: column Kw is the constant 1 of the bias gradient
    long long M, T, HW;              // rows, rows per chunk, rows per image
    float* part;                     // [chunks][N][Kp]
};

__global__ __launch_bounds__(256) void ops_wgrad_kernel(const WgP P)
{
    __shared__ __attribute__((aligned(16))) float As[GK][GAP];
    __shared__ __attribute__((aligned(16))) float Bs[GK][GN];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * GM, k0 = blockIdx.y * GN;
    const long long tb = (long long)blockIdx.z * P.T, te = tb + P.T < P.M ? tb + P.T : P.M;

    const int an = n0 + (tid & 127);            // the dz column this thread stages, at tokens (tid >> 7) + 2 i
    const bool aok = an < P.N;
    const int kc = k0 + (tid & 63);             // the A column this thread stages, at tokens (tid >> 6) + 4 i
    const bool kok = kc < P.Kw, one = kc == P.Kw;
    int ci = 0, dyy = 0, dxx = 0;
    if (P.conv && kok) {
        const int tap = kc / P.cin;
        ci = kc - tap * P.cin;
        dyy = tap / 3 - 1;
        dxx = tap % 3 - 1;
    }
    float av[8], bv[4];
    auto load = [&](long long t0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long long t = t0 + (tid >> 7) + 2 * i;
            av[i] = (aok && t < te) ? P.dz[t * P.N + an] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long t = t0 + (tid >> 6) + 4 * i;
            float v = 0.f;
            if (t < te) {
                if (one) v = 1.f;
                else if (kok) {
                    if (!P.conv) v = P.a[t * P.Kw + kc];
                    else {
                        const long long b = t / P.HW, p = t - b * P.HW;
                        const int y = (int)(p / P.W), x = (int)(p - (long long)y * P.W);
                        const int yy = y + dyy, xx = x + dxx;
                        if (yy >= 0 && yy < P.H && xx >= 0 && xx < P.W) v = P.a[(b * P.HW + (long long)yy * P.W + xx) * P.cin + ci];
                    }
                }
            }
            bv[i] = v;
        }
    };

    // thread (ty, tx) owns rows 8 ty .. 8 ty + 7 and columns 4 tx .. 4 tx + 3 of the 128 x 64 tile: every product joins a double sum
    double acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    const int ty = tid >> 4, tx = tid & 15;
    load(tb);
    for (long long t0 = tb; t0 < te; t0 += GK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) As[(tid >> 7) + 2 * i][tid & 127] = av[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[(tid >> 6) + 4 * i][tid & 63] = bv[i];
        __syncthreads();
        if (t0 + GK < te) load(t0 + GK);
        tile_fma(As, Bs, ty, tx, acc);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = n0 + 8 * ty + i;
        if (n >= P.N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * tx + j;
            if (k < P.Kp) P.part[((long long)blockIdx.z * P.N + n) * P.Kp + k] = (float)acc[i][j];
        }
    }
}

// dw[co][ci][tap] = sum over the chunks, ascending, of part[c][co][tap cin + ci]; db[co] of column Kw.  One thread per output.
__global__ __launch_bounds__(256) void ops_wgrad_reduce_kernel(const float* part, int chunks, int N, int cin, int taps, float* dw, float* db)
{
    const int Kw = cin * taps, Kp = Kw + 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, nw = (long long)N * Kw;
    if (i >= nw + N) return;
    int co, col;
    float* dst;
    if (i < nw) {
        co = (int)(i / Kw);
        const int r = (int)(i - (long long)co * Kw), ci = r / taps, t = r - ci * taps;
        col = t * cin + ci;
        dst = dw ? dw + i : nullptr;
    } else {
        co = (int)(i - nw);
        col = Kw;
        dst = db ? db + co : nullptr;
    }
    if (!dst) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += (double)part[((long long)c * N + co) * Kp + col];
    *dst = (float)s;
}

// the weight of the input-gradient conv: wT[(tp cout + co) cin + ci] = w[co][ci][8 - tp]
__global__ __launch_bounds__(256) void ops_flip_kernel(const float* w, float* wT, int cout, int cin)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 9ll * cout * cin) return;
    const int ci = (int)(i % cin);
    const long long r = i / cin;
    const int co = (int)(r % cout), tp = (int)(r / cout);
    wT[i] = w[((long long)co * cin + ci) * 9 + (8 - tp)];
}

// out[i] = sum over c of part[c stride + i], one wave per output: lane l takes c = l, l + 64, .. in ascending order, then a fixed
// exchange tree.  Outputs [0, n1) go to out1, [n1, n) to out2.
__global__ __launch_bounds__(256) void ops_reduce_wave_kernel(const float* part, long long nc, long long stride, long long n, long long n1,
                                                              float* out1, float* out2)
{
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    double s = 0.0;
    for (long long c = lane; c < nc; c += 64) s += (double)part[c * stride + i];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        if (i < n1) out1[i] = (float)s;
        else out2[i - n1] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm backward
// ---------------------------------------------------------------------------------------------------------------
// one wave per token: dx = (g - mean(g) - xhat mean(g xhat)) / sd with g = dy w, everything in double; stats[m] = (mean, 1 / sd)
__global__ __launch_bounds__(256) void ops_ln_bwd_kernel(const float* dy, const float* x, const float* w, float* dx, double2* stats, long long M, int C)
{
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const float* xr = x + m * C;
    const float* gr = dy + m * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)xr[c];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    const double mu = s / C;
    double q = 0.0;
    for (int c = lane; c < C; c += 64) { const double d = (double)xr[c] - mu; q = fma(d, d, q); }
    for (int o = 32; o; o >>= 1) q += __shfl_xor(q, o);
    const double rstd = 1.0 / sqrt(q / C + 1e-5);
    double s1 = 0.0, s2 = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double g = (double)gr[c] * (double)w[c];
        s1 += g;
        s2 = fma(g, ((double)xr[c] - mu) * rstd, s2);
    }
    for (int o = 32; o; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    s1 /= C;
    s2 /= C;
    if (dx)
        for (int c = lane; c < C; c += 64) {
            const double g = (double)gr[c] * (double)w[c], xh = ((double)xr[c] - mu) * rstd;
            dx[m * C + c] = (float)((g - s1 - xh * s2) * rstd);
        }
    if (stats && lane == 0) stats[m] = make_double2(mu, rstd);
}

// part[ch][0][c] = sum over the LN_ROWS rows of chunk ch, ascending, of dy xhat; part[ch][1][c] of dy.  One thread per channel.
__global__ __launch_bounds__(64) void ops_ln_wgrad_kernel(const float* dy, const float* x, const double2* stats, float* part, long long M, int C)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const long long mb = (long long)blockIdx.y * LN_ROWS, me = mb + LN_ROWS < M ? mb + LN_ROWS : M;
    double sg = 0.0, sb = 0.0;
    for (long long m = mb; m < me; ++m) {
        const double2 st = stats[m];
        const double g = (double)dy[m * C + c];
        sg = fma(g, ((double)x[m * C + c] - st.x) * st.y, sg);
        sb += g;
    }
    part[((long long)blockIdx.y * 2) * C + c] = (float)sg;
    part[((long long)blockIdx.y * 2 + 1) * C + c] = (float)sb;
}

// ---------------------------------------------------------------------------------------------------------------
// window attention backward
// ---------------------------------------------------------------------------------------------------------------
struct AttnBP {
    const float* qkv;            // as AttnP
    const float* dout;           // token rows of C
    const float* table;
    float* dqkv;                 // token rows of 3 C; every element is written
    float* tpart;                // [B nw][(2 ws - 1)^2][heads]
    int H, W, C, heads, hd, ws, shift, nwx, nw;
    float scale;
};

constexpr int AB_R = 8;          // query rows per block of P / dS in LDS: 32 lanes per row

template <int NT>
__global__ __launch_bounds__(256) void ops_attn_bwd_kernel(const AttnBP P)
{
    constexpr int NP = NT * 32;
    __shared__ float Qs[NP][33];             // q scale
    __shared__ float Ks[NP][33];
    __shared__ float Vs[NP][33];
    __shared__ float Gs[NP][33];             // d out
    __shared__ float Ps[AB_R][NP + 1];
    __shared__ float Ds[AB_R][NP + 1];       // dS
    const int tid = threadIdx.x;
    const int ws = P.ws, N = ws * ws, h = blockIdx.y, hd = P.hd;
    const int b = (int)blockIdx.x / P.nw, win = (int)blockIdx.x - b * P.nw;
    const int wy = win / P.nwx, wx = win - wy * P.nwx;
    const long long HW = (long long)P.H * P.W;
    const int C3 = 3 * P.C;
    auto tok = [&](int i) -> long long {
        const int iy = i / ws, ix = i - iy * ws;
        const int y = (wy * ws + iy + P.shift) % P.H, x = (wx * ws + ix + P.shift) % P.W;
        return (long long)b * HW + (long long)y * P.W + x;
    };
    for (int e = tid; e < NP * 32; e += 256) {
        const int j = e >> 5, d = e & 31;
        float qv = 0.f, kv = 0.f, vv = 0.f, gv = 0.f;
        if (j < N && d < hd) {
            const long long t = tok(j);
            const float* row = P.qkv + t * C3 + h * hd + d;
            qv = row[0] * P.scale;
            kv = row[P.C];
            vv = row[2 * P.C];
            gv = P.dout[t * P.C + h * hd + d];
        }
        Qs[j][d] = qv;
        Ks[j][d] = kv;
        Vs[j][d] = vv;
        Gs[j][d] = gv;
    }
    __syncthreads();

    const int r = tid >> 5, sub = tid & 31, side = 2 * ws - 1, bins = side * side;
    double dk[4 * NT], dv[4 * NT], tb[4];
#pragma unroll
    for (int u = 0; u < 4 * NT; ++u) { dk[u] = 0.0; dv[u] = 0.0; }
#pragma unroll
    for (int u = 0; u < 4; ++u) tb[u] = 0.0;

    for (int i0 = 0; i0 < N; i0 += AB_R) {
        const int i = i0 + r;
        const bool iok = i < N;
        const int ie = iok ? i : 0;          // a row past the window computes row 0 and stores zeros: no lane leaves the exchanges
        const int qy = ie / ws, qx = ie - qy * ws;
        const int qreg = P.shift ? 3 * region(wy * ws + qy, P.H, ws, P.shift) + region(wx * ws + qx, P.W, ws, P.shift) : 0;
        double p[NT], ds[NT];
        double mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int j = sub + 32 * u;
            double s = -INFINITY;
            if (j < N) {
                double acc = 0.0;
                for (int d = 0; d < hd; ++d) acc = fma((double)Ks[j][d], (double)Qs[ie][d], acc);
                const int ky = j / ws, kx = j - ky * ws;
                s = acc + (double)P.table[((qy - ky + ws - 1) * side + (qx - kx + ws - 1)) * P.heads + h];
                if (P.shift) {
                    const int kreg = 3 * region(wy * ws + ky, P.H, ws, P.shift) + region(wx * ws + kx, P.W, ws, P.shift);
                    if (kreg != qreg) s += -100.0;
                }
            }
            p[u] = s;
            mx = fmax(mx, s);
        }
        for (int o = 16; o; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        double den = 0.0;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int j = sub + 32 * u;
            p[u] = j < N ? exp(p[u] - mx) : 0.0;
            den += p[u];
        }
        for (int o = 16; o; o >>= 1) den += __shfl_xor(den, o);
        double delta = 0.0;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int j = sub + 32 * u;
            p[u] /= den;
            double acc = 0.0;
            if (j < N)
                for (int d = 0; d < hd; ++d) acc = fma((double)Gs[ie][d], (double)Vs[j][d], acc);
            ds[u] = acc;                                   // dP
            delta = fma(acc, p[u], delta);
        }
        for (int o = 16; o; o >>= 1) delta += __shfl_xor(delta, o);
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int j = sub + 32 * u;
            Ps[r][j] = iok ? (float)p[u] : 0.f;
            Ds[r][j] = iok ? (float)(p[u] * (ds[u] - delta)) : 0.f;
        }
        __syncthreads();
        // dq of this row block: thread (r, d = sub)
        if (iok && sub < hd) {
            double acc = 0.0;
            for (int j = 0; j < N; ++j) acc = fma((double)Ds[r][j], (double)Ks[j][sub], acc);
            P.dqkv[tok(i) * C3 + h * hd + sub] = (float)(acc * (double)P.scale);
        }
        // dk, dv: thread owns (key (tid >> 5) + 8 u, channel tid & 31) and adds this block's rows in ascending order
#pragma unroll 1
        for (int rr = 0; rr < AB_R; ++rr) {
            const double qd = (double)Qs[i0 + rr][sub], gd = (double)Gs[i0 + rr][sub];
#pragma unroll
            for (int u = 0; u < 4 * NT; ++u) {
                dk[u] = fma((double)Ds[rr][r + 8 * u], qd, dk[u]);
                dv[u] = fma((double)Ps[rr][r + 8 * u], gd, dv[u]);
            }
        }
        // the table: thread owns bins tid + 256 u; for each row the one key that maps to the bin
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int bin = tid + 256 * u;
            if (bin < bins) {
                const int by = bin / side, oy = by - (ws - 1), ox = bin - by * side - (ws - 1);
                for (int rr = 0; rr < AB_R && i0 + rr < N; ++rr) {
                    const int iy = (i0 + rr) / ws, ix = (i0 + rr) - iy * ws;
                    const int ky = iy - oy, kx = ix - ox;
                    if (ky >= 0 && ky < ws && kx >= 0 && kx < ws) tb[u] += (double)Ds[rr][ky * ws + kx];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4 * NT; ++u) {
        const int jj = r + 8 * u;
        if (jj < N && sub < hd) {
            float* row = P.dqkv + tok(jj) * C3 + h * hd + sub;
            row[P.C] = (float)dk[u];
            row[2 * P.C] = (float)dv[u];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int bin = tid + 256 * u;
        if (bin < bins) P.tpart[((long long)blockIdx.x * bins + bin) * P.heads + h] = (float)tb[u];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

// rows per weight-gradient chunk: the caller's, or enough chunks to fill the device a few times over
long long wgrad_rows(long long M, int N, int Kp, long long chunk)
{
    if (chunk > 0) return chunk;
    const long long tiles = (long long)((N + GM - 1) / GM) * ((Kp + GN - 1) / GN);
    const long long want = std::max(1ll, 1024 / tiles);
    long long T = std::max(256ll, (M + want - 1) / want);
    return (T + GK - 1) / GK * GK;
}

struct LinShape { int conv, B, H, W, cin, N, act; long long M, chunk; };

int check_lin(const char* op, const LinShape& s, int math)
{
    if (math == 3)
        return rfail(XSD_ERR_ARG, "%s: math mode bf16x6 is not supported by the differentiable ops (fp32 only)", op);
    if (math != 0) return rfail(XSD_ERR_ARG, "%s: unknown math mode %d; the differentiable ops run in fp32 (0) only", op, math);
    if (s.conv) {
        if (s.B < 1 || s.H < 1 || s.W < 1 || (long long)s.B * s.H * s.W > OPS_MAX_ROWS)
            return rfail(XSD_ERR_ARG, "%s: %d images of %d x %d pixels are outside [1, 2^28] rows", op, s.B, s.H, s.W);
    } else if (s.M < 1 || s.M > OPS_MAX_ROWS) {
        return rfail(XSD_ERR_ARG, "%s: %lld rows are outside [1, 2^28]", op, s.M);
    }
    if (s.cin < 1 || s.cin > 65536 || s.N < 1 || s.N > 65536)
        return rfail(XSD_ERR_ARG, "%s: %d inputs and %d outputs are outside [1, 65536]", op, s.cin, s.N);
    if (s.act < ACT_NONE || s.act > ACT_LRELU) return rfail(XSD_ERR_ARG, "%s: activation %d (0 none, 1 GELU, 2 LeakyReLU)", op, s.act);
    if (s.chunk < 0) return rfail(XSD_ERR_ARG, "%s: a weight-gradient chunk of %lld rows is negative (0 = the default)", op, s.chunk);
    return XSD_OK;
}

// scratch of the backward: [dz (act != none)] [flipped weight (conv)] [weight-gradient partials]
struct LinPlan { long long dz = 0, wT = 0, part = 0, bytes = 0, T = 0; int chunks = 0, Kw = 0, Kp = 0; };

int plan_lin(const char* op, const LinShape& s, bool backward, LinPlan& pl)
{
    const long long M = s.conv ? (long long)s.B * s.H * s.W : s.M;
    pl.Kw = s.cin * (s.conv ? 9 : 1);
    pl.Kp = pl.Kw + 1;
    if ((long long)s.cin * (s.conv ? 9 : 1) > (1 << 24)) return rfail(XSD_ERR_ARG, "%s: %d inputs are too many for a 3x3 conv", op, s.cin);
    if (!backward) { pl.bytes = al256(sizeof(float) * (long long)pl.Kw * s.N); return XSD_OK; }
    pl.T = wgrad_rows(M, s.N, pl.Kp, s.chunk);
    const long long chunks = (M + pl.T - 1) / pl.T;
    if (chunks > OPS_MAX_CHUNKS)
        return rfail(XSD_ERR_ARG, "%s: a weight-gradient chunk of %lld rows splits %lld rows into %lld partials; at most %d", op, pl.T, M, chunks,
                     OPS_MAX_CHUNKS);
    pl.chunks = (int)chunks;
    long long off = 0;
    pl.dz = off; off += s.act != ACT_NONE ? al256(sizeof(float) * M * s.N) : 0;
    pl.wT = off; off += s.conv ? al256(sizeof(float) * 9ll * s.N * s.cin) : 0;
    pl.part = off; off += al256(sizeof(float) * chunks * s.N * pl.Kp);
    pl.bytes = off;
    return XSD_OK;
}

int lin_forward(const char* op, const LinShape& s, int math, const float* a, const float* w, const float* bias, float* y, float* z, float slope,
                void* scratch, long long scratch_bytes, hipStream_t st)
{
    int rc = check_lin(op, s, math);
    if (rc) return rc;
    if (!a || !w || !y || !scratch) return rfail(XSD_ERR_ARG, "%s: null argument", op);
    LinPlan pl;
    if ((rc = plan_lin(op, s, false, pl))) return rc;
    if (scratch_bytes < pl.bytes) return rfail(XSD_ERR_ARG, "%s: scratch of %lld bytes; %lld are needed", op, scratch_bytes, pl.bytes);
    const long long M = s.conv ? (long long)s.B * s.H * s.W : s.M, wn = (long long)s.N * pl.Kw;
    float* wp = (float*)scratch;
    hipLaunchKernelGGL(sw_pack_kernel, dim3(blocks256(wn)), dim3(256), 0, st, w, wp, s.N, s.cin, s.conv ? 9 : 1);
    hipError_t e = hipGetLastError();
    if (!e) {
        const bool split = z && s.act != ACT_NONE;         // the pre-activation is kept: y = act(z) by the epilogue's own expression
        e = s.conv ? conv(st, a, s.B, s.H, s.W, s.cin, wp, s.N, bias, split ? ACT_NONE : s.act, slope, split ? z : y)
                   : conv(st, a, 1, 1, (int)M, s.cin, wp, s.N, bias, split ? ACT_NONE : s.act, slope, split ? z : y, 1);
        if (!e && split) {
            hipLaunchKernelGGL(ops_act_kernel, dim3(blocks256(M * s.N)), dim3(256), 0, st, z, y, M * s.N, s.act, slope);
            e = hipGetLastError();
        }
    }
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", op, hipGetErrorString(e));
    return XSD_OK;
}

int lin_backward(const char* op, const LinShape& s, int math, const float* dy, const float* a, const float* w, const float* z, float* da, float* dw,
                 float* db, float slope, void* scratch, long long scratch_bytes, hipStream_t st)
{
    int rc = check_lin(op, s, math);
    if (rc) return rc;
    if (!dy || !a || !w || !scratch || (s.act != ACT_NONE && !z)) return rfail(XSD_ERR_ARG, "%s: null argument", op);
    LinPlan pl;
    if ((rc = plan_lin(op, s, true, pl))) return rc;
    if (scratch_bytes < pl.bytes) return rfail(XSD_ERR_ARG, "%s: scratch of %lld bytes; %lld are needed", op, scratch_bytes, pl.bytes);
    const long long M = s.conv ? (long long)s.B * s.H * s.W : s.M;
    char* base = (char*)scratch;
    const float* dz = dy;
    hipError_t e = hipSuccess;
    if (s.act != ACT_NONE) {
        float* t = (float*)(base + pl.dz);
        hipLaunchKernelGGL(ops_act_bwd_kernel, dim3(blocks256(M * s.N)), dim3(256), 0, st, dy, z, t, M * s.N, s.act, slope);
        e = hipGetLastError();
        dz = t;
    }
    if (!e && da) {
        if (s.conv) {
            float* wT = (float*)(base + pl.wT);
            hipLaunchKernelGGL(ops_flip_kernel, dim3(blocks256(9ll * s.N * s.cin)), dim3(256), 0, st, w, wT, s.N, s.cin);
            e = hipGetLastError();
            if (!e) e = conv(st, dz, s.B, s.H, s.W, s.N, wT, s.cin, nullptr, ACT_NONE, 0.f, da);
        } else {
            // the stored [N][cin] weight is the [K'][N'] matrix of dz W
            e = conv(st, dz, 1, 1, (int)M, s.N, w, s.cin, nullptr, ACT_NONE, 0.f, da, 1);
        }
    }
    if (!e && (dw || db)) {
        WgP p{};
        p.dz = dz; p.N = s.N; p.a = a; p.conv = s.conv; p.H = s.conv ? s.H : 1; p.W = s.conv ? s.W : 1; p.cin = s.cin; p.Kw = pl.Kw; p.Kp = pl.Kp;
        p.M = M; p.T = pl.T; p.HW = s.conv ? (long long)s.H * s.W : 1;
        p.part = (float*)(base + pl.part);
        dim3 grid((unsigned)((s.N + GM - 1) / GM), (unsigned)((pl.Kp + GN - 1) / GN), (unsigned)pl.chunks);
        hipLaunchKernelGGL(ops_wgrad_kernel, grid, dim3(256), 0, st, p);
        e = hipGetLastError();
        if (!e) {
            hipLaunchKernelGGL(ops_wgrad_reduce_kernel, dim3(blocks256((long long)s.N * pl.Kp)), dim3(256), 0, st, p.part, pl.chunks, s.N, s.cin,
                               s.conv ? 9 : 1, dw, db);
            e = hipGetLastError();
        }
    }
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", op, hipGetErrorString(e));
    return XSD_OK;
}

int check_ln(const char* op, long long M, int C)
{
    if (M < 1 || M > (1ll << 31)) return rfail(XSD_ERR_ARG, "%s: %lld rows are outside [1, 2^31]", op, M);
    if (C < 1 || C > 4096) return rfail(XSD_ERR_ARG, "%s: %d channels are outside [1, 4096]", op, C);
    return XSD_OK;
}

int check_attn(const char* op, int B, int H, int W, int C, int heads, int ws, int shift)
{
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "%s: bad shape %dx%dx%d", op, B, H, W);
    if (ws < 1 || ws > 16) return rfail(XSD_ERR_ARG, "%s: window size %d is outside [1, 16] (256 tokens per window)", op, ws);
    if (H % ws || W % ws) return rfail(XSD_ERR_ARG, "%s: H and W must be multiples of the window size %d; got %d x %d", op, ws, H, W);
    if (shift < 0 || shift >= ws) return rfail(XSD_ERR_ARG, "%s: shift %d is outside [0, window size %d)", op, shift, ws);
    if (heads < 1 || heads > 65535 || C < 1 || C % heads) return rfail(XSD_ERR_ARG, "%s: %d heads do not divide %d channels", op, heads, C);
    if (C / heads > 32) return rfail(XSD_ERR_ARG, "%s: head dim %d; the kernel takes at most 32", op, C / heads);
    if ((long long)B * (H / ws) * (W / ws) > 0x7fffffffll || (long long)B * H * W > OPS_MAX_ROWS)
        return rfail(XSD_ERR_ARG, "%s: %d images of %d x %d tokens are too many", op, B, H, W);
    return XSD_OK;
}

long long attn_scratch(int B, int H, int W, int heads, int ws)
{
    const long long side = 2 * ws - 1;
    return al256(sizeof(float) * (long long)B * (H / ws) * (W / ws) * side * side * heads);
}

} // namespace

extern "C" {

int64_t xsd_sw_op_linear_scratch(int64_t M, int K, int N, int act, int64_t chunk, int backward)
{
    const LinShape s{0, 1, 1, 1, K, N, act, M, chunk};
    LinPlan pl;
    if (check_lin("linear", s, 0) || plan_lin("linear", s, backward != 0, pl)) return -1;
    return pl.bytes;
}

int xsd_sw_op_linear_forward(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, float* dev_z, int64_t M, int K, int N,
                             int act, float slope, int math, void* scratch, int64_t scratch_bytes, void* stream)
{
    const LinShape s{0, 1, 1, 1, K, N, act, M, 0};
    return lin_forward("linear", s, math, dev_a, dev_w, dev_bias, dev_y, dev_z, slope, scratch, scratch_bytes, (hipStream_t)stream);
}

int xsd_sw_op_linear_backward(const float* dev_dy, const float* dev_a, const float* dev_w, const float* dev_z, float* dev_da, float* dev_dw,
                              float* dev_db, int64_t M, int K, int N, int act, float slope, int math, int64_t chunk, void* scratch,
                              int64_t scratch_bytes, void* stream)
{
    const LinShape s{0, 1, 1, 1, K, N, act, M, chunk};
    return lin_backward("linear", s, math, dev_dy, dev_a, dev_w, dev_z, dev_da, dev_dw, dev_db, slope, scratch, scratch_bytes, (hipStream_t)stream);
}

int64_t xsd_sw_op_conv3x3_scratch(int B, int H, int W, int cin, int N, int act, int64_t chunk, int backward)
{
    const LinShape s{1, B, H, W, cin, N, act, 0, chunk};
    LinPlan pl;
    if (check_lin("conv3x3", s, 0) || plan_lin("conv3x3", s, backward != 0, pl)) return -1;
    return pl.bytes;
}

int xsd_sw_op_conv3x3_forward(const float* dev_x, const float* dev_w, const float* dev_bias, float* dev_y, float* dev_z, int B, int H, int W,
                              int cin, int N, int act, float slope, int math, void* scratch, int64_t scratch_bytes, void* stream)
{
    const LinShape s{1, B, H, W, cin, N, act, 0, 0};
    return lin_forward("conv3x3", s, math, dev_x, dev_w, dev_bias, dev_y, dev_z, slope, scratch, scratch_bytes, (hipStream_t)stream);
}

int xsd_sw_op_conv3x3_backward(const float* dev_dy, const float* dev_x, const float* dev_w, const float* dev_z, float* dev_dx, float* dev_dw,
                               float* dev_db, int B, int H, int W, int cin, int N, int act, float slope, int math, int64_t chunk, void* scratch,
                               int64_t scratch_bytes, void* stream)
{
    const LinShape s{1, B, H, W, cin, N, act, 0, chunk};
    return lin_backward("conv3x3", s, math, dev_dy, dev_x, dev_w, dev_z, dev_dx, dev_dw, dev_db, slope, scratch, scratch_bytes, (hipStream_t)stream);
}

int xsd_sw_op_layernorm_forward(const float* dev_x, const float* dev_w, const float* dev_b, float* dev_y, int64_t M, int C, void* stream)
{
    if (!dev_x || !dev_w || !dev_b || !dev_y) return rfail(XSD_ERR_ARG, "layer_norm: null argument");
    int rc = check_ln("layer_norm", M, C);
    if (rc) return rc;
    hipError_t e = ln((hipStream_t)stream, dev_x, dev_y, dev_w, dev_b, M, C);
    if (e) return rfail(XSD_ERR_HIP, "layer_norm: %s", hipGetErrorString(e));
    return XSD_OK;
}

int64_t xsd_sw_op_layernorm_scratch(int64_t M, int C)
{
    if (check_ln("layer_norm", M, C)) return -1;
    return al256(sizeof(double2) * M) + al256(sizeof(float) * ((M + LN_ROWS - 1) / LN_ROWS) * 2 * C);
}

int xsd_sw_op_layernorm_backward(const float* dev_dy, const float* dev_x, const float* dev_w, float* dev_dx, float* dev_dw, float* dev_db,
                                 int64_t M, int C, void* scratch, int64_t scratch_bytes, void* stream)
{
    if (!dev_dy || !dev_x || !dev_w || !scratch) return rfail(XSD_ERR_ARG, "layer_norm: null argument");
    if ((dev_dw == nullptr) != (dev_db == nullptr)) return rfail(XSD_ERR_ARG, "layer_norm: the gradients of weight and bias come together");
    int rc = check_ln("layer_norm", M, C);
    if (rc) return rc;
    const long long need = xsd_sw_op_layernorm_scratch(M, C);
    if (scratch_bytes < need) return rfail(XSD_ERR_ARG, "layer_norm: scratch of %lld bytes; %lld are needed", (long long)scratch_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    double2* stats = (double2*)scratch;
    float* part = (float*)((char*)scratch + al256(sizeof(double2) * M));
    const long long chunks = (M + LN_ROWS - 1) / LN_ROWS;
    if (dev_dw && chunks > 65535)
        return rfail(XSD_ERR_ARG, "layer_norm: %lld rows are too many for the weight gradient (at most %d)", (long long)M, 65535 * LN_ROWS);
    hipLaunchKernelGGL(ops_ln_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, dev_dy, dev_x, dev_w, dev_dx, dev_dw ? stats : nullptr, M, C);
    hipError_t e = hipGetLastError();
    if (!e && dev_dw) {
        hipLaunchKernelGGL(ops_ln_wgrad_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)chunks), dim3(64), 0, s, dev_dy, dev_x, stats, part, M, C);
        e = hipGetLastError();
        if (!e) {
            hipLaunchKernelGGL(ops_reduce_wave_kernel, dim3((unsigned)((2 * C + 3) / 4)), dim3(256), 0, s, part, chunks, 2ll * C, 2ll * C, (long long)C,
                               dev_dw, dev_db);
            e = hipGetLastError();
        }
    }
    if (e) return rfail(XSD_ERR_HIP, "layer_norm: %s", hipGetErrorString(e));
    return XSD_OK;
}

int xsd_sw_op_attention_forward(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws,
                                int shift, float scale, void* stream)
{
    if (!dev_qkv || !dev_table || !dev_out) return rfail(XSD_ERR_ARG, "window_attention: null argument");
    int rc = check_attn("window_attention", B, H, W, C, heads, ws, shift);
    if (rc) return rc;
    hipError_t e = attention((hipStream_t)stream, dev_qkv, dev_out, dev_table, B, H, W, C, heads, ws, shift, scale);
    if (e) return rfail(XSD_ERR_HIP, "window_attention: %s", hipGetErrorString(e));
    return XSD_OK;
}

int64_t xsd_sw_op_attention_scratch(int B, int H, int W, int C, int heads, int ws)
{
    if (check_attn("window_attention", B, H, W, C, heads, ws, 0)) return -1;
    return attn_scratch(B, H, W, heads, ws);
}

int xsd_sw_op_attention_backward(const float* dev_dout, const float* dev_qkv, const float* dev_table, float* dev_dqkv, float* dev_dtable, int B,
                                 int H, int W, int C, int heads, int ws, int shift, float scale, void* scratch, int64_t scratch_bytes, void* stream)
{
    if (!dev_dout || !dev_qkv || !dev_table || !dev_dqkv || !dev_dtable || !scratch) return rfail(XSD_ERR_ARG, "window_attention: null argument");
    int rc = check_attn("window_attention", B, H, W, C, heads, ws, shift);
    if (rc) return rc;
    const long long need = attn_scratch(B, H, W, heads, ws);
    if (scratch_bytes < need) return rfail(XSD_ERR_ARG, "window_attention: scratch of %lld bytes; %lld are needed", (long long)scratch_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    AttnBP p{};
    p.qkv = dev_qkv; p.dout = dev_dout; p.table = dev_table; p.dqkv = dev_dqkv; p.tpart = (float*)scratch;
    p.H = H; p.W = W; p.C = C; p.heads = heads; p.hd = C / heads; p.ws = ws; p.shift = shift;
    p.nwx = W / ws; p.nw = (H / ws) * p.nwx;
    p.scale = scale;
    dim3 grid((unsigned)(B * p.nw), (unsigned)heads);
    switch ((ws * ws + 31) / 32) {
#define OPS_ATT(T) case T: hipLaunchKernelGGL(ops_attn_bwd_kernel<T>, grid, dim3(256), 0, s, p); break;
    OPS_ATT(1) OPS_ATT(2) OPS_ATT(3) OPS_ATT(4) OPS_ATT(5) OPS_ATT(6) OPS_ATT(7) OPS_ATT(8)
#undef OPS_ATT
    default: return rfail(XSD_ERR_ARG, "window_attention: window size %d is outside [1, 16]", ws);
    }
    hipError_t e = hipGetLastError();
    if (!e) {
        const long long side = 2 * ws - 1, n = side * side * heads;
        hipLaunchKernelGGL(ops_reduce_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, p.tpart, (long long)B * p.nw, n, n, n, dev_dtable,
                           dev_dtable);
        e = hipGetLastError();
    }
    if (e) return rfail(XSD_ERR_HIP, "window_attention: %s", hipGetErrorString(e));
    return XSD_OK;
}

} // extern "C"
