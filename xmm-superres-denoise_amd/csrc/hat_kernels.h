// hat_kernels.h -- the kernels HAT has on top of sw_kernels.h that more than one translation unit launches, with the host code that
// launches them: the overlapping cross-attention of the OCAB and the two stages of the channel attention's gates.  hat.hip (the fused
// eval forward and the xsd_hat_test_* hooks) and hat_ops.hip (the differentiable ops overlap_attention and channel_attention) each
// compile their own instance, as sw_kernels.h and sw_fft.h are shared.  Include after sw_kernels.h, or after <hip/hip_runtime.h>,
// <algorithm>, <cmath> and its f32x16.  hat.hip's header comment
// describes the three kernels.
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------------------------
// overlapping cross-attention
// ---------------------------------------------------------------------------------------------------------------
constexpr int OC_KC = 64;        // keys per LDS chunk (two 32-key MFMA tiles)
constexpr int OC_MAX_OW = 32;    // the overlapping window side the index arithmetic and the launch are checked for

struct OcaP {
    const float* qkv;            // token rows of 3 C: q, k, v; head h at channels h hd .. h hd + hd - 1 of each (hat.py:334-368)
    float* o;                    // token rows of C
    const float* table;          // relative_position_bias_table [(ws + ow - 1)^2][heads]
    int H, W, C, heads, hd, ws, ow, pad, nwx, nw;
    float scale;
};

__global__ __launch_bounds__(512) void hat_ocab_kernel(const OcaP P)
{
    __shared__ float Ks[OC_KC][33];
    __shared__ float Vs[OC_KC][32];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, i32 = lane & 31, h2 = lane >> 5;
    const int ws = P.ws, ow = P.ow, NQ = ws * ws, NK = ow * ow, h = blockIdx.y;
    const int b = (int)blockIdx.x / P.nw, win = (int)blockIdx.x - b * P.nw;
    const int wy = win / P.nwx, wx = win - wy * P.nwx;
    const long long HW = (long long)P.H * P.W;
    const int C3 = 3 * P.C;
    const int qi = 32 * wave + i32;
    const bool qok = qi < NQ;
    const int qy = qi / ws, qx = qi - qy * ws;
    float qv[16];
    {
        const float* row = P.qkv + (qok ? (long long)b * HW + (long long)(wy * ws + qy) * P.W + wx * ws + qx : 0) * C3 + h * P.hd;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int d = 2 * s + h2;
            qv[s] = (qok && d < P.hd) ? row[d] * P.scale : 0.f;        // q = q * self.scale (hat.py:370)
        }
    }
    // key j of the overlapping window = pixel (wy ws - pad + j / ow, wx ws - pad + j % ow), a zero vector outside the image
    auto stage = [&](int j0, bool with_v) {
        for (int e = tid; e < OC_KC * 32; e += nthr) {
            const int jl = e >> 5, d = e & 31, j = j0 + jl;
            float kv = 0.f, vv = 0.f;
            if (j < NK && d < P.hd) {
                const int ky = j / ow, kx = j - ky * ow;
                const int y = wy * ws - P.pad + ky, x = wx * ws - P.pad + kx;
                if (y >= 0 && y < P.H && x >= 0 && x < P.W) {
                    const float* row = P.qkv + ((long long)b * HW + (long long)y * P.W + x) * C3 + h * P.hd + d;
                    kv = row[P.C];
                    if (with_v) vv = row[2 * P.C];
                }
            }
            Ks[jl][d] = kv;
            if (with_v) Vs[jl][d] = vv;
        }
    };
    // S^T = K (q scale)^T of one 32-key tile plus the bias: acc[v] of lane l = S[query 32 wave + l % 32][key j0 + 32 t + 8 (v / 4) +
    // 4 (l / 32) + v % 4]; keys past the window's last are -inf
    const int side = ws + ow - 1, tsize = side * side, off = ws - ow + 1;
    auto scores = [&](int t, int j0, f32x16& acc) {
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (2 * s >= P.hd) break;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[32 * t + i32][2 * s + h2], qv[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int j = j0 + 32 * t + 8 * (v >> 2) + 4 * h2 + (v & 3);
            if (j >= NK) acc[v] = -INFINITY;
            else if (qok) {
                const int ky = j / ow, kx = j - ky * ow;
                int idx = (ky - qy + off) * side + (kx - qx + off);            // calculate_rpi_oca (hat.py:820-833)
                if (idx < 0) idx += tsize;                                      // table[negative index] counts from the end
                acc[v] += P.table[idx * P.heads + h];
            }
        }
    };
    f32x16 acc;
    float mx = -INFINITY;
    for (int j0 = 0; j0 < NK; j0 += OC_KC) {
        __syncthreads();
        stage(j0, false);
        __syncthreads();
        for (int t = 0; t < OC_KC / 32 && j0 + 32 * t < NK; ++t) {
            scores(t, j0, acc);
#pragma unroll
            for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    // per chunk of 64 keys the sum of exp and P V are fp32 chains from zero (P V on the MFMA); the chunks are summed in double
    double den = 0.0, od[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) od[v] = 0.0;
    for (int j0 = 0; j0 < NK; j0 += OC_KC) {
        __syncthreads();
        stage(j0, true);
        __syncthreads();
        float dc = 0.f;
        f32x16 o;
#pragma unroll
        for (int v = 0; v < 16; ++v) o[v] = 0.f;
        for (int t = 0; t < OC_KC / 32 && j0 + 32 * t < NK; ++t) {
            scores(t, j0, acc);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float e = expf(acc[v] - mx);
                acc[v] = e;
                dc += e;
            }
#pragma unroll
            for (int v = 0; v < 16; ++v)
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[v], Vs[32 * t + 8 * (v >> 2) + 4 * h2 + (v & 3)][i32], o, 0, 0, 0);
        }
        den += (double)dc;
#pragma unroll
        for (int v = 0; v < 16; ++v) od[v] += (double)o[v];
    }
    den += __shfl_xor(den, 32);
    // od[v] of lane l = sum_j e[query r][j] v[j][d = l % 32], r = 8 (v / 4) + 4 (l / 32) + v % 4 of this wave; its denominator is lane r's
    double dn[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) dn[v] = __shfl(den, 8 * (v >> 2) + 4 * h2 + (v & 3));
    if (i32 >= P.hd) return;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int q = 32 * wave + 8 * (v >> 2) + 4 * h2 + (v & 3);
        if (q >= NQ) continue;
        const int oy = q / ws, ox = q - oy * ws;
        P.o[((long long)b * HW + (long long)(wy * ws + oy) * P.W + wx * ws + ox) * P.C + h * P.hd + i32] = (float)(od[v] / dn[v]);
    }
}

hipError_t ocab(hipStream_t s, const float* qkv, float* out, const float* table, int B, int H, int W, int C, int heads, int ws, int ow,
                float scale)
{
    OcaP p{};
    p.qkv = qkv; p.o = out; p.table = table;
    p.H = H; p.W = W; p.C = C; p.heads = heads; p.hd = C / heads; p.ws = ws; p.ow = ow; p.pad = (ow - ws) / 2;
    p.nwx = W / ws; p.nw = (H / ws) * p.nwx;
    p.scale = scale;
    const int nqt = (ws * ws + 31) / 32;
    hipLaunchKernelGGL(hat_ocab_kernel, dim3((unsigned)(B * p.nw), (unsigned)heads), dim3(64 * nqt), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// channel attention
// ---------------------------------------------------------------------------------------------------------------
constexpr int PL_ROWS = 256;     // pixels per partial sum: the chunking depends on H W alone, never on the batch

// x: token-major [B][HW][C]; part: [B][nchunk][C] doubles
__global__ __launch_bounds__(256) void hat_pool_partial_kernel(const float* x, double* part, long long HW, int C, int nchunk)
{
    const int b = blockIdx.y, ch = blockIdx.x;
    const long long r0 = (long long)ch * PL_ROWS, r1 = r0 + PL_ROWS < HW ? r0 + PL_ROWS : HW;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float* p = x + ((long long)b * HW + r0) * C + c;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        long long r = r0;
        for (; r + 4 <= r1; r += 4) {
            s0 += (double)p[0];
            s1 += (double)p[C];
            s2 += (double)p[2ll * C];
            s3 += (double)p[3ll * C];
            p += 4ll * C;
        }
        for (; r < r1; ++r) { s0 += (double)p[0]; p += C; }
        part[((long long)b * nchunk + ch) * C + c] = (s0 + s1) + (s2 + s3);
    }
}

// w1 [Cs][C], w2 [C][Cs] (the 1x1 conv weights as stored); mean_out [B][C] or null; y [B][C] or null (then only the means are made)
__global__ __launch_bounds__(256) void hat_ca_kernel(const double* part, int nchunk, long long HW, int C, int Cs, const float* w1,
                                                     const float* b1, const float* w2, const float* b2, float* mean_out, float* y)
{
    extern __shared__ float ca_sm[];
    float* mean = ca_sm;
    float* hid = ca_sm + C;
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int k = 0; k < nchunk; ++k) s += part[((long long)b * nchunk + k) * C + c];
        const float m = (float)(s / (double)HW);
        mean[c] = m;
        if (mean_out) mean_out[(long long)b * C + c] = m;
    }
    if (!y) return;
    __syncthreads();
    for (int j = threadIdx.x; j < Cs; j += 256) {
        double a = 0.0;
        for (int c = 0; c < C; ++c) a = fma((double)w1[(long long)j * C + c], (double)mean[c], a);
        const float v = (float)a + b1[j];
        hid[j] = v < 0.f ? 0.f : v;                                   // ReLU (a NaN stays a NaN)
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double a = 0.0;
        for (int j = 0; j < Cs; ++j) a = fma((double)w2[(long long)c * Cs + j], (double)hid[j], a);
        const float v = (float)a + b2[c];
        y[(long long)b * C + c] = 1.f / (1.f + expf(-v));
    }
}

int pool_chunks(long long HW) { return (int)((HW + PL_ROWS - 1) / PL_ROWS); }

hipError_t pool_partial(hipStream_t s, const float* x, double* part, int B, long long HW, int C)
{
    const int nchunk = pool_chunks(HW);
    hipLaunchKernelGGL(hat_pool_partial_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, s, x, part, HW, C, nchunk);
    return hipGetLastError();
}

// the gates y [B][C] (and / or the means) from the partial sums of pool_partial
hipError_t ca(hipStream_t s, const double* part, int B, long long HW, int C, int Cs, const float* w1, const float* b1, const float* w2,
              const float* b2, float* mean_out, float* y)
{
    hipLaunchKernelGGL(hat_ca_kernel, dim3((unsigned)B), dim3(256), sizeof(float) * (size_t)(C + std::max(Cs, 1)), s, part, pool_chunks(HW), HW, C,
                       Cs, w1, b1, w2, b2, mean_out, y);
    return hipGetLastError();
}

} // namespace
