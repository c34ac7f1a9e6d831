// hat_ops.hip -- the two operations HAT has on top of the differentiable Swin ops (sw_ops.hip), as stand-alone differentiable ops
// (include/xsd.h, "differentiable HAT ops"): overlap_attention, the overlapping cross-attention of the OCAB between its qkv Linear and
// proj (hat.py:334-391), and channel_attention, the gate at the end of the CAB (hat.py:20-29).  One forward and one backward entry
// each, for the torch.autograd.Functions of xmm_superres_denoise/ops.py that models/modules/hat_train.py composes.
//
// The forwards run hat_kernels.h's kernels with the arguments of the xsd_hat_test_* hooks (this file compiles its own instance of
// them, as hat.hip does): out is bitwise xsd_hat_test_ocab's, the gates are bitwise xsd_hat_test_ca_combine's dev_y.  The gate is
// applied by hat_ca_scale_kernel, out of place.
// The backwards follow sw_ops.hip's rules: every product an exact fp32 product added in double, no float atomics, every reduction in
// a fixed order, nothing allocated and nothing synchronised: scratch is the caller's.  One exception to "added in double", as in
// sw_ops.hip's ops_attn_bwd_kernel: P and dS of a block pass through LDS as fp32 (one more rounding per element) before they are
// summed in double into dq, dk, dv and the table bins; the op tests hold the result to the bar.
//   overlap_attention  hat_ocab_bwd_kernel, one workgroup of 256 threads per (window, head).  The probabilities are recomputed from
//                      qkv; no ws^2 x ow^2 matrix is kept.  Eight query rows at a time (32 lanes per row) against the forward's
//                      chunks of 64 keys.  Phase Q, per row block: the row's maximum and denominator in one sweep over the chunks
//                      (the running pair rescaled in double), delta = dout . out from the saved output, then a second sweep with
//                      dS = p (dP - delta) of a chunk in LDS, from which dq (thread = (row, channel), carried across the chunks) and
//                      the bias-table bins (each thread owns its bins and looks up, per row, the one key that reads it; the
//                      negative indices wrap as in the forward; the padded keys are keys like any other here).  The rows' maximum,
//                      denominator and delta stay in LDS.  Phase K, per chunk of keys: all row blocks again, P and dS of a block in
//                      LDS, dk / dv carried in registers (thread = (key, channel), rows ascending) and written as the (window, head)'s
//                      slab.  A token is a key of up to ceil(ow / ws)^2 windows: hat_ocab_kv_gather_kernel sums its slabs in ascending
//                      window order into the k and v thirds of dqkv.  Out-of-image keys are zero vectors: their slab rows are never read.
//   channel_attention  hat_ca_dg_partial_kernel (per image, channel and the pool's chunk of 256 pixels: the sum of t, by the pool's
//                      own four chains, and the sum of dy t), hat_ca_bwd_kernel (one workgroup per image: the mean, the squeeze MLP and
//                      the gate recomputed and differentiated in double -- the forward's fp32 gate would hand its rounding to dt --
//                      per-image partials of the four parameter gradients, g and dmean), hat_ca_reduce_kernel (the images in
//                      ascending order), hat_ca_dt_kernel (dt = dy g + dmean / HW, rounded once).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/xsd.h"

#include "xsd_err.h"
#define rfail xsd::failf      // the thread-local message of xsd_last_error()

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));       // sw_kernels.h's, which this file does not need otherwise
}

#include "hat_kernels.h"

namespace {

long long al256(long long bytes) { return (bytes + 255) & ~255ll; }
unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

// ---------------------------------------------------------------------------------------------------------------
// overlapping cross-attention, backward
// ---------------------------------------------------------------------------------------------------------------
constexpr int OB_R = 8;          // query rows per block of P / dS in LDS: 32 lanes per row
constexpr int OB_BINS = 9;       // bias-table bins per thread: (16 + 32 - 1)^2 = 2209 <= 9 * 256
constexpr int OB_NOBIN = 1 << 20;

struct OcaBP {
    const float* qkv;            // as OcaP
    const float* dout;           // token rows of C
    const float* out;            // the forward's output, token rows of C
    const float* table;
    float* dqkv;                 // token rows of 3 C; this kernel writes the q third
    float* slab;                 // [B nw][ow^2][2][C]: dk, dv of every (window, key)
    float* tpart;                // [B nw][(ws + ow - 1)^2][heads]
    int H, W, C, heads, hd, ws, ow, pad, nwx, nw;
    float scale;
};

__global__ __launch_bounds__(256) void hat_ocab_bwd_kernel(const OcaBP P)
{
    __shared__ float Ks[OC_KC][33];
    __shared__ float Vs[OC_KC][33];
    __shared__ float Qb[OB_R][33];            // q scale
    __shared__ float Gb[OB_R][33];            // d out
    __shared__ float Ps[OB_R][OC_KC + 1];
    __shared__ float Ds[OB_R][OC_KC + 1];     // dS
    __shared__ double Mx[256], Dn[256], Dl[256];
    const int tid = threadIdx.x, r = tid >> 5, sub = tid & 31;
    const int ws = P.ws, ow = P.ow, NQ = ws * ws, NK = ow * ow, h = blockIdx.y, hd = P.hd;
    const int b = (int)blockIdx.x / P.nw, win = (int)blockIdx.x - b * P.nw;
    const int wy = win / P.nwx, wx = win - wy * P.nwx;
    const long long HW = (long long)P.H * P.W;
    const int C3 = 3 * P.C;
    const int side = ws + ow - 1, tsize = side * side, off = ws - ow + 1;
    auto qtok = [&](int i) -> long long {
        const int iy = i / ws, ix = i - iy * ws;
        return (long long)b * HW + (long long)(wy * ws + iy) * P.W + wx * ws + ix;
    };
    // key j of the overlapping window = pixel (wy ws - pad + j / ow, wx ws - pad + j % ow), a zero vector outside the image
    auto stage_kv = [&](int j0) {
        for (int e = tid; e < OC_KC * 32; e += 256) {
            const int jl = e >> 5, d = e & 31, j = j0 + jl;
            float kv = 0.f, vv = 0.f;
            if (j < NK && d < hd) {
                const int ky = j / ow, kx = j - ky * ow;
                const int y = wy * ws - P.pad + ky, x = wx * ws - P.pad + kx;
                if (y >= 0 && y < P.H && x >= 0 && x < P.W) {
                    const float* row = P.qkv + ((long long)b * HW + (long long)y * P.W + x) * C3 + h * hd + d;
                    kv = row[P.C];
                    vv = row[2 * P.C];
                }
            }
            Ks[jl][d] = kv;
            Vs[jl][d] = vv;
        }
    };
    // thread (r, sub) stages channel sub of query row i0 + r; a row past the window's last is staged as zeros.  -> this lane's dout * out
    auto stage_q = [&](int i0) -> double {
        const int i = i0 + r;
        float qv = 0.f, gv = 0.f, ov = 0.f;
        if (i < NQ && sub < hd) {
            const long long t = qtok(i);
            qv = P.qkv[t * C3 + h * hd + sub] * P.scale;
            gv = P.dout[t * P.C + h * hd + sub];
            ov = P.out[t * P.C + h * hd + sub];
        }
        Qb[r][sub] = qv;
        Gb[r][sub] = gv;
        return (double)gv * (double)ov;
    };
    // the score of query (qy, qx), staged as row r, against key j = j0 + jl of the staged chunk
    auto score = [&](int qy, int qx, int j, int jl) -> double {
        double acc = 0.0;
        for (int d = 0; d < hd; ++d) acc = fma((double)Ks[jl][d], (double)Qb[r][d], acc);
        const int ky = j / ow, kx = j - ky * ow;
        int idx = (ky - qy + off) * side + (kx - qx + off);
        if (idx < 0) idx += tsize;
        return acc + (double)P.table[idx * P.heads + h];
    };

    // the bins this thread owns: bin = tid + 256 u.  idx = a side + c with a = ky - qy + off and c = kx - qx + off, both in
    // [2 - ow, ws]: side values, so (a, c) -> idx is one to one, and so is the wrap of the negative ones (they land above ws (side + 1))
    int bdy[OB_BINS], bdx[OB_BINS];
    double tb[OB_BINS];
#pragma unroll
    for (int u = 0; u < OB_BINS; ++u) {
        const int bin = tid + 256 * u, lo = 2 - ow;
        bdy[u] = OB_NOBIN;
        bdx[u] = 0;
        tb[u] = 0.0;
        if (bin < tsize) {
            for (int cand = 0; cand < 2; ++cand) {
                const int v = bin - cand * tsize;
                const int c = lo + (((v - lo) % side) + side) % side;
                const int a = (v - c) / side;
                if (a >= lo && a <= ws) { bdy[u] = a - off; bdx[u] = c - off; }
            }
        }
    }

    // ---- phase Q: row statistics, dq, the table ----
    for (int i0 = 0; i0 < NQ; i0 += OB_R) {
        __syncthreads();
        double delta = stage_q(i0);
        for (int o = 16; o; o >>= 1) delta += __shfl_xor(delta, o);
        __syncthreads();
        const int i = i0 + r;
        const bool iok = i < NQ;
        const int ie = iok ? i : 0;              // a row past the window computes on zeros and stores zeros: no lane leaves the exchanges
        const int qy = ie / ws, qx = ie - qy * ws;
        double m = -INFINITY, den = 0.0;
        for (int j0 = 0; j0 < NK; j0 += OC_KC) {
            __syncthreads();
            stage_kv(j0);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int jl = sub + 32 * u, j = j0 + jl;
                if (j < NK) {
                    const double s = score(qy, qx, j, jl);
                    if (s > m) {
                        den = den * exp(m - s) + 1.0;          // m = -inf: den is 0 and stays 0
                        m = s;
                    } else {
                        den += exp(s - m);                     // a NaN score lands here and stays
                    }
                }
            }
        }
        for (int o = 16; o; o >>= 1) {
            const double m2 = __shfl_xor(m, o), d2 = __shfl_xor(den, o);
            const double mn = fmax(m, m2);
            den = (m == -INFINITY ? 0.0 : den * exp(m - mn)) + (m2 == -INFINITY ? 0.0 : d2 * exp(m2 - mn));
            m = mn;
        }
        if (sub == 0) { Mx[i0 + r] = m; Dn[i0 + r] = den; Dl[i0 + r] = delta; }
        double dq = 0.0;
        for (int j0 = 0; j0 < NK; j0 += OC_KC) {
            __syncthreads();
            stage_kv(j0);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int jl = sub + 32 * u, j = j0 + jl;
                float df = 0.f;
                if (j < NK && iok) {
                    const double p = exp(score(qy, qx, j, jl) - m) / den;
                    double dp = 0.0;
                    for (int d = 0; d < hd; ++d) dp = fma((double)Gb[r][d], (double)Vs[jl][d], dp);
                    df = (float)(p * (dp - delta));
                }
                Ds[r][jl] = df;
            }
            __syncthreads();
            if (sub < hd)
                for (int jl = 0; jl < OC_KC; ++jl) dq = fma((double)Ds[r][jl], (double)Ks[jl][sub], dq);
#pragma unroll
            for (int u = 0; u < OB_BINS; ++u) {
                if (bdy[u] == OB_NOBIN) continue;
                for (int rr = 0; rr < OB_R && i0 + rr < NQ; ++rr) {
                    const int iy = (i0 + rr) / ws, ix = (i0 + rr) - iy * ws;
                    const int ky = iy + bdy[u], kx = ix + bdx[u];
                    if (ky < 0 || ky >= ow || kx < 0 || kx >= ow) continue;
                    const int jl = ky * ow + kx - j0;
                    if (jl >= 0 && jl < OC_KC) tb[u] += (double)Ds[rr][jl];
                }
            }
        }
        if (iok && sub < hd) P.dqkv[qtok(i) * C3 + h * hd + sub] = (float)(dq * (double)P.scale);
    }
#pragma unroll
    for (int u = 0; u < OB_BINS; ++u) {
        const int bin = tid + 256 * u;
        if (bin < tsize) P.tpart[((long long)blockIdx.x * tsize + bin) * P.heads + h] = (float)tb[u];
    }

    // ---- phase K: dk, dv of every key of the overlapping window ----
    for (int j0 = 0; j0 < NK; j0 += OC_KC) {
        __syncthreads();
        stage_kv(j0);
        double dk[OC_KC / OB_R], dv[OC_KC / OB_R];
#pragma unroll
        for (int u = 0; u < OC_KC / OB_R; ++u) { dk[u] = 0.0; dv[u] = 0.0; }
        for (int i0 = 0; i0 < NQ; i0 += OB_R) {
            __syncthreads();
            (void)stage_q(i0);
            __syncthreads();
            const int i = i0 + r;
            const bool iok = i < NQ;
            const int ie = iok ? i : 0;
            const int qy = ie / ws, qx = ie - qy * ws;
            const double m = Mx[i0 + r], den = Dn[i0 + r], delta = Dl[i0 + r];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int jl = sub + 32 * u, j = j0 + jl;
                float pf = 0.f, df = 0.f;
                if (j < NK && iok) {
                    const double p = exp(score(qy, qx, j, jl) - m) / den;
                    double dp = 0.0;
                    for (int d = 0; d < hd; ++d) dp = fma((double)Gb[r][d], (double)Vs[jl][d], dp);
                    pf = (float)p;
                    df = (float)(p * (dp - delta));
                }
                Ps[r][jl] = pf;
                Ds[r][jl] = df;
            }
            __syncthreads();
            // thread owns (key r + 8 u, channel sub) and adds this block's rows in ascending order
#pragma unroll 1
            for (int rr = 0; rr < OB_R; ++rr) {
                const double qd = (double)Qb[rr][sub], gd = (double)Gb[rr][sub];
#pragma unroll
                for (int u = 0; u < OC_KC / OB_R; ++u) {
                    dk[u] = fma((double)Ds[rr][r + OB_R * u], qd, dk[u]);
                    dv[u] = fma((double)Ps[rr][r + OB_R * u], gd, dv[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < OC_KC / OB_R; ++u) {
            const int j = j0 + r + OB_R * u;
            if (j < NK && sub < hd) {
                float* row = P.slab + (((long long)blockIdx.x * NK + j) * 2) * P.C + h * hd + sub;
                row[0] = (float)dk[u];
                row[P.C] = (float)dv[u];
            }
        }
    }
}

// dqkv[token][C + c] (k) and [2 C + c] (v): the token's slab rows of every window whose overlapping window holds it, in ascending
// window order, summed in double.  One thread per (token, k / v, channel).
__global__ __launch_bounds__(256) void hat_ocab_kv_gather_kernel(const float* slab, float* dqkv, int H, int W, int C, int ws, int ow, int pad,
                                                                 int nwy, int nwx, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int C2 = 2 * C, NK = ow * ow;
    const int c2 = (int)(i % C2);
    const long long t = i / C2, HW = (long long)H * W;
    const long long b = t / HW, p = t - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const int kv = c2 / C, c = c2 - kv * C;
    // window row wy holds image row y as key row y + pad - wy ws, which must lie in [0, ow)
    const int ny = y + pad - ow + 1, nx = x + pad - ow + 1;
    const int wy0 = ny <= 0 ? 0 : (ny + ws - 1) / ws, wy1 = min(nwy - 1, (y + pad) / ws);
    const int wx0 = nx <= 0 ? 0 : (nx + ws - 1) / ws, wx1 = min(nwx - 1, (x + pad) / ws);
    double s = 0.0;
    for (int wy = wy0; wy <= wy1; ++wy)
        for (int wx = wx0; wx <= wx1; ++wx) {
            const int ky = y + pad - wy * ws, kx = x + pad - wx * ws;
            const long long win = (b * nwy + wy) * nwx + wx;
            s += (double)slab[((win * NK + ky * ow + kx) * 2 + kv) * C + c];
        }
    dqkv[t * 3 * C + (1 + kv) * C + c] = (float)s;
}

// out[i] = sum over c of part[c stride + i], one wave per output: lane l takes c = l, l + 64, .. in ascending order, then a fixed
// exchange tree (sw_ops.hip's reduction of the window attention's table partials)
__global__ __launch_bounds__(256) void hat_reduce_wave_kernel(const float* part, long long nc, long long stride, long long n, float* out)
{
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    double s = 0.0;
    for (long long c = lane; c < nc; c += 64) s += (double)part[c * stride + i];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[i] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------
// channel attention
// ---------------------------------------------------------------------------------------------------------------
// y[i] = t[i] * g[b][c], i = (b HW + p) C + c
__global__ __launch_bounds__(256) void hat_ca_scale_kernel(const float* t, const float* g, float* y, long long HWC, int C, long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    y[i] = t[i] * g[(i / HWC) * C + (int)(i % C)];
}

// part [B][nchunk][2][C] doubles: [0] the sum of t over the chunk's pixels by hat_pool_partial_kernel's four chains,
// [1] the sum of dy t
__global__ __launch_bounds__(256) void hat_ca_dg_partial_kernel(const float* dy, const float* t, double* part, long long HW, int C, int nchunk)
{
    const int b = blockIdx.y, ch = blockIdx.x;
    const long long r0 = (long long)ch * PL_ROWS, r1 = r0 + PL_ROWS < HW ? r0 + PL_ROWS : HW;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float* p = t + ((long long)b * HW + r0) * C + c;
        const float* g = dy + ((long long)b * HW + r0) * C + c;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
        long long r = r0;
        for (; r + 4 <= r1; r += 4) {
            s0 += (double)p[0];
            s1 += (double)p[C];
            s2 += (double)p[2ll * C];
            s3 += (double)p[3ll * C];
            d0 = fma((double)g[0], (double)p[0], d0);
            d1 = fma((double)g[C], (double)p[C], d1);
            d2 = fma((double)g[2ll * C], (double)p[2ll * C], d2);
            d3 = fma((double)g[3ll * C], (double)p[3ll * C], d3);
            p += 4ll * C;
            g += 4ll * C;
        }
        for (; r < r1; ++r) {
            s0 += (double)p[0];
            d0 = fma((double)g[0], (double)p[0], d0);
            p += C;
            g += C;
        }
        double* o = part + (((long long)b * nchunk + ch) * 2) * C + c;
        o[0] = (s0 + s1) + (s2 + s3);
        o[C] = (d0 + d1) + (d2 + d3);
    }
}

// One workgroup per image.  The mean, the hidden vector and the gate are recomputed in double from the chunk sums (the forward rounds
// each to fp32; the backward differentiates the exact function, so dt and the parameter gradients carry one rounding):
// g = sigmoid(w2 relu(w1 mean + b1) + b2); dz = dg g (1 - g); db2 = dz; dw2[c][j] = dz[c] hid[j]; dhid = w2^T dz; dv = dhid where the
// pre-activation is > 0, 0 where it is not, the NaN where it is one; db1 = dv; dw1[j][c] = dv[j] mean[c]; dmean = w1^T dv.
// vecs: this image's vectors, 3 C + Cs doubles: [mean (C)][g (C)][dmean (C)][pre-activation (Cs)].
// pimg: this image's partials, n = 2 Cs C + Cs + C doubles: [dw1 (Cs C)][db1 (Cs)][dw2 (C Cs)][db2 (C)].
__global__ __launch_bounds__(256) void hat_ca_bwd_kernel(const double* part, int nchunk, long long HW, int C, int Cs, const float* w1,
                                                         const float* b1, const float* w2, const float* b2, double* vecs, double* pimg)
{
    const int b = blockIdx.x;
    const long long CsC = (long long)Cs * C;
    double* mean = vecs + (long long)b * (3 * C + Cs);
    double* gd = mean + C;
    double* dmean = gd + C;
    double* pre = dmean + C;
    double* pw1 = pimg + (long long)b * (2 * CsC + Cs + C);
    double* dv = pw1 + CsC;              // db1
    double* pw2 = dv + Cs;
    double* dz = pw2 + CsC;              // db2; until the gate is known it holds dg
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0, dg = 0.0;
        for (int k = 0; k < nchunk; ++k) {
            const double* q = part + (((long long)b * nchunk + k) * 2) * C + c;
            s += q[0];
            dg += q[C];
        }
        mean[c] = s / (double)HW;
        dz[c] = dg;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Cs; j += 256) {
        double a = 0.0;
        for (int c = 0; c < C; ++c) a = fma((double)w1[(long long)j * C + c], mean[c], a);
        pre[j] = a + (double)b1[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double a = 0.0;
        for (int j = 0; j < Cs; ++j) a = fma((double)w2[(long long)c * Cs + j], pre[j] < 0.0 ? 0.0 : pre[j], a);      // ReLU (a NaN stays a NaN)
        const double g = 1.0 / (1.0 + exp(-(a + (double)b2[c])));
        gd[c] = g;
        dz[c] = dz[c] * (g * (1.0 - g));
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Cs; j += 256) {
        double dh = 0.0;
        for (int c = 0; c < C; ++c) dh = fma((double)w2[(long long)c * Cs + j], dz[c], dh);
        const double v = pre[j];
        dv[j] = v > 0.0 ? dh : (v == v ? 0.0 : v);
    }
    __syncthreads();
    for (long long e = threadIdx.x; e < CsC; e += 256) {
        const int c = (int)(e / Cs), j = (int)(e - (long long)c * Cs);
        pw2[e] = dz[c] * (pre[j] < 0.0 ? 0.0 : pre[j]);
        const int j1 = (int)(e / C), c1 = (int)(e - (long long)j1 * C);
        pw1[e] = dv[j1] * mean[c1];
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        double a = 0.0;
        for (int j = 0; j < Cs; ++j) a = fma((double)w1[(long long)j * C + c], dv[j], a);
        dmean[c] = a;
    }
}

// the per-image partials summed over the images in ascending order; one thread per element of [dw1][db1][dw2][db2]
__global__ __launch_bounds__(256) void hat_ca_reduce_kernel(const double* pimg, int B, long long n, long long n1, long long n2, long long n3,
                                                            float* dw1, float* db1, float* dw2, float* db2)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += pimg[(long long)b * n + i];
    if (i < n1) dw1[i] = (float)s;
    else if (i < n2) db1[i - n1] = (float)s;
    else if (i < n3) dw2[i - n2] = (float)s;
    else db2[i - n3] = (float)s;
}

// dt[i] = dy[i] g[b][c] + dmean[b][c] / HW, in double with hat_ca_bwd_kernel's g and dmean (vecs), rounded once
__global__ __launch_bounds__(256) void hat_ca_dt_kernel(const float* dy, const double* vecs, float* dt, long long HW, long long HWC, int C, int Cs,
                                                        long long total)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const double* v = vecs + (i / HWC) * (3 * C + Cs) + (int)(i % C);
    dt[i] = (float)fma((double)dy[i], v[C], v[2 * C] / (double)HW);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
const char* const OA = "overlap_attention";
const char* const CA = "channel_attention";

int check_ocab(int B, int H, int W, int C, int heads, int ws, int ow)
{
    if (B < 1 || H < 1 || W < 1) return rfail(XSD_ERR_ARG, "%s: bad shape %dx%dx%d", OA, B, H, W);
    if (ws < 1 || ws > 16) return rfail(XSD_ERR_ARG, "%s: window size %d is outside [1, 16] (256 queries per window)", OA, ws);
    if (ow < ws || ow > OC_MAX_OW)
        return rfail(XSD_ERR_ARG, "%s: overlap window %d is outside [window size %d, %d] (1024 keys per window)", OA, ow, ws, OC_MAX_OW);
    if ((ow - ws) % 2) return rfail(XSD_ERR_ARG, "%s: overlap window %d minus window size %d is odd (the padding is half of it)", OA, ow, ws);
    if (ws * (ws + ow) >= (ws + ow - 1) * (ws + ow - 1))
        return rfail(XSD_ERR_ARG, "%s: window size %d with an overlap window of %d indexes past the bias table", OA, ws, ow);
    if (H % ws || W % ws) return rfail(XSD_ERR_ARG, "%s: H and W must be multiples of the window size %d; got %d x %d", OA, ws, H, W);
    if (heads < 1 || heads > 65535 || C < 1 || C % heads) return rfail(XSD_ERR_ARG, "%s: %d heads do not divide %d channels", OA, heads, C);
    if (C / heads > 32) return rfail(XSD_ERR_ARG, "%s: head dim %d; the kernel takes at most 32", OA, C / heads);
    if ((long long)B * (H / ws) * (W / ws) > 0x7fffffffll || (long long)B * H * W > (1ll << 28))
        return rfail(XSD_ERR_ARG, "%s: %d images of %d x %d tokens are too many", OA, B, H, W);
    if ((long long)B * H * W * C > (1ll << 37))      // the gather runs one thread per (token, k / v, channel): 2^38 / 256 blocks at most
        return rfail(XSD_ERR_ARG, "%s: %d x %d x %d tokens of %d channels are too many elements (at most 2^37)", OA, B, H, W, C);
    return XSD_OK;
}

// scratch of the backward: [dk / dv slabs: B nw x ow^2 x 2 C floats] [table partials: B nw x (ws + ow - 1)^2 x heads floats]
struct OcaPlan { long long slab, tpart, bytes; };

OcaPlan plan_ocab(int B, int H, int W, int C, int heads, int ws, int ow)
{
    const long long nwin = (long long)B * (H / ws) * (W / ws), side = ws + ow - 1;
    OcaPlan pl{};
    pl.slab = 0;
    pl.tpart = al256(sizeof(float) * nwin * ow * ow * 2 * C);
    pl.bytes = pl.tpart + al256(sizeof(float) * nwin * side * side * heads);
    return pl;
}

int check_ca(int B, long long HW, int C, int Cs)
{
    if (B < 1 || B > 65535) return rfail(XSD_ERR_ARG, "%s: %d images are outside [1, 65535]", CA, B);
    if (HW < 1 || HW > (1ll << 28)) return rfail(XSD_ERR_ARG, "%s: %lld pixels are outside [1, 2^28]", CA, HW);
    if (C < 1 || C > 4096) return rfail(XSD_ERR_ARG, "%s: %d channels are outside [1, 4096]", CA, C);
    if (Cs < 1 || Cs > 4096) return rfail(XSD_ERR_ARG, "%s: a squeezed width of %d is outside [1, 4096]", CA, Cs);
    if ((long long)B * HW * C > (1ll << 38)) return rfail(XSD_ERR_ARG, "%s: %d x %lld x %d elements are too many", CA, B, HW, C);
    return XSD_OK;
}

// scratch: forward [pool partials: B x chunks x C doubles] [the gates, where the caller takes none: B x C floats]; backward [partials of t and dy t: B x chunks x 2 C doubles]
// [per-image vectors mean, g, dmean, hidden pre-activation: B x (3 C + Cs) doubles] [per-image parameter partials: B x (2 Cs C + Cs + C) doubles]
struct CaPlan { long long vecs, pimg, bytes; };

CaPlan plan_ca(int B, long long HW, int C, int Cs, bool backward)
{
    const long long chunks = pool_chunks(HW);
    CaPlan pl{};
    if (!backward) {
        pl.vecs = al256(sizeof(double) * B * chunks * C);         // here: the gates
        pl.bytes = pl.vecs + al256(sizeof(float) * (long long)B * C);
        return pl;
    }
    pl.vecs = al256(sizeof(double) * B * chunks * 2 * C);
    pl.pimg = pl.vecs + al256(sizeof(double) * (long long)B * (3 * C + Cs));
    pl.bytes = pl.pimg + al256(sizeof(double) * B * (2ll * Cs * C + Cs + C));
    return pl;
}

} // namespace

extern "C" {

int xsd_hat_op_ocab_forward(const float* dev_qkv, const float* dev_table, float* dev_out, int B, int H, int W, int C, int heads, int ws, int ow,
                            float scale, void* stream)
{
    if (!dev_qkv || !dev_table || !dev_out) return rfail(XSD_ERR_ARG, "%s: null argument", OA);
    if (int rc = check_ocab(B, H, W, C, heads, ws, ow)) return rc;
    hipError_t e = ocab((hipStream_t)stream, dev_qkv, dev_out, dev_table, B, H, W, C, heads, ws, ow, scale);
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", OA, hipGetErrorString(e));
    return XSD_OK;
}

int64_t xsd_hat_op_ocab_scratch(int B, int H, int W, int C, int heads, int ws, int ow)
{
    if (check_ocab(B, H, W, C, heads, ws, ow)) return -1;
    return plan_ocab(B, H, W, C, heads, ws, ow).bytes;
}

int xsd_hat_op_ocab_backward(const float* dev_dout, const float* dev_qkv, const float* dev_table, const float* dev_out, float* dev_dqkv,
                             float* dev_dtable, int B, int H, int W, int C, int heads, int ws, int ow, float scale, void* scratch,
                             int64_t scratch_bytes, void* stream)
{
    if (!dev_dout || !dev_qkv || !dev_table || !dev_out || !dev_dqkv || !dev_dtable || !scratch) return rfail(XSD_ERR_ARG, "%s: null argument", OA);
    if (int rc = check_ocab(B, H, W, C, heads, ws, ow)) return rc;
    const OcaPlan pl = plan_ocab(B, H, W, C, heads, ws, ow);
    if (scratch_bytes < pl.bytes) return rfail(XSD_ERR_ARG, "%s: scratch of %lld bytes; %lld are needed", OA, (long long)scratch_bytes, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    OcaBP p{};
    p.qkv = dev_qkv; p.dout = dev_dout; p.out = dev_out; p.table = dev_table; p.dqkv = dev_dqkv;
    p.slab = (float*)((char*)scratch + pl.slab);
    p.tpart = (float*)((char*)scratch + pl.tpart);
    p.H = H; p.W = W; p.C = C; p.heads = heads; p.hd = C / heads; p.ws = ws; p.ow = ow; p.pad = (ow - ws) / 2;
    p.nwx = W / ws; p.nw = (H / ws) * p.nwx;
    p.scale = scale;
    hipLaunchKernelGGL(hat_ocab_bwd_kernel, dim3((unsigned)(B * p.nw), (unsigned)heads), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (!e) {
        const long long total = (long long)B * H * W * 2 * C;
        hipLaunchKernelGGL(hat_ocab_kv_gather_kernel, dim3(blocks256(total)), dim3(256), 0, s, p.slab, dev_dqkv, H, W, C, ws, ow, p.pad, H / ws,
                           p.nwx, total);
        e = hipGetLastError();
    }
    if (!e) {
        const long long side = ws + ow - 1, n = side * side * heads;
        hipLaunchKernelGGL(hat_reduce_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, p.tpart, (long long)B * p.nw, n, n, dev_dtable);
        e = hipGetLastError();
    }
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", OA, hipGetErrorString(e));
    return XSD_OK;
}

int xsd_hat_op_ca_forward(const float* dev_t, const float* dev_w1, const float* dev_b1, const float* dev_w2, const float* dev_b2, float* dev_y,
                          float* dev_gates, int B, int64_t HW, int C, int Cs, void* scratch, int64_t scratch_bytes, void* stream)
{
    if (!dev_t || !dev_w1 || !dev_b1 || !dev_w2 || !dev_b2 || !dev_y || !scratch) return rfail(XSD_ERR_ARG, "%s: null argument", CA);
    if (int rc = check_ca(B, HW, C, Cs)) return rc;
    const CaPlan pl = plan_ca(B, HW, C, Cs, false);
    if (scratch_bytes < pl.bytes) return rfail(XSD_ERR_ARG, "%s: scratch of %lld bytes; %lld are needed", CA, (long long)scratch_bytes, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    if (!dev_gates) dev_gates = (float*)((char*)scratch + pl.vecs);
    hipError_t e = pool_partial(s, dev_t, part, B, HW, C);
    if (!e) e = ca(s, part, B, HW, C, Cs, dev_w1, dev_b1, dev_w2, dev_b2, nullptr, dev_gates);
    if (!e) {
        const long long total = (long long)B * HW * C;
        hipLaunchKernelGGL(hat_ca_scale_kernel, dim3(blocks256(total)), dim3(256), 0, s, dev_t, dev_gates, dev_y, HW * C, C, total);
        e = hipGetLastError();
    }
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", CA, hipGetErrorString(e));
    return XSD_OK;
}

int64_t xsd_hat_op_ca_scratch(int B, int64_t HW, int C, int Cs, int backward)
{
    if (check_ca(B, HW, C, Cs)) return -1;
    return plan_ca(B, HW, C, Cs, backward != 0).bytes;
}

int xsd_hat_op_ca_backward(const float* dev_dy, const float* dev_t, const float* dev_w1, const float* dev_b1, const float* dev_w2,
                           const float* dev_b2, float* dev_dt, float* dev_dw1, float* dev_db1, float* dev_dw2, float* dev_db2,
                           int B, int64_t HW, int C, int Cs, void* scratch, int64_t scratch_bytes, void* stream)
{
    if (!dev_dy || !dev_t || !dev_w1 || !dev_b1 || !dev_w2 || !dev_b2 || !dev_dt || !dev_dw1 || !dev_db1 || !dev_dw2 || !dev_db2 ||
        !scratch)
        return rfail(XSD_ERR_ARG, "%s: null argument", CA);
    if (int rc = check_ca(B, HW, C, Cs)) return rc;
    const CaPlan pl = plan_ca(B, HW, C, Cs, true);
    if (scratch_bytes < pl.bytes) return rfail(XSD_ERR_ARG, "%s: scratch of %lld bytes; %lld are needed", CA, (long long)scratch_bytes, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    double* vecs = (double*)((char*)scratch + pl.vecs);
    double* pimg = (double*)((char*)scratch + pl.pimg);
    const int nchunk = pool_chunks(HW);
    hipLaunchKernelGGL(hat_ca_dg_partial_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, s, dev_dy, dev_t, part, (long long)HW, C, nchunk);
    hipError_t e = hipGetLastError();
    if (!e) {
        hipLaunchKernelGGL(hat_ca_bwd_kernel, dim3((unsigned)B), dim3(256), 0, s, part, nchunk, (long long)HW, C, Cs, dev_w1, dev_b1, dev_w2, dev_b2,
                           vecs, pimg);
        e = hipGetLastError();
    }
    if (!e) {
        const long long CsC = (long long)Cs * C, n = 2 * CsC + Cs + C;
        hipLaunchKernelGGL(hat_ca_reduce_kernel, dim3(blocks256(n)), dim3(256), 0, s, pimg, B, n, CsC, CsC + Cs, 2 * CsC + Cs, dev_dw1, dev_db1,
                           dev_dw2, dev_db2);
        e = hipGetLastError();
    }
    if (!e) {
        const long long total = (long long)B * HW * C;
        hipLaunchKernelGGL(hat_ca_dt_kernel, dim3(blocks256(total)), dim3(256), 0, s, dev_dy, vecs, dev_dt, (long long)HW, HW * C, C, Cs, total);
        e = hipGetLastError();
    }
    if (e) return rfail(XSD_ERR_HIP, "%s: %s", CA, hipGetErrorString(e));
    return XSD_OK;
}

} // extern "C"
