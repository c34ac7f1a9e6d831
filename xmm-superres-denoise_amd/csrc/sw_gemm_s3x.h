// sw_gemm_s3x.h -- the "bf16x6" (strict split) form of sw_kernels.h's GEMM, the opt-in math mode 3 of the SwinFIR, HAT and SwinIR engines.
//
// Same GemmP, same A modes (token rows; implicit im2col of a 3x3 conv over NCHW or token-major input with the input affine), same
// epilogues and stores as sw_gemm_kernel.  Every fp32 operand is split EXACTLY into hi + mid + lo bf16 (xsd_split.h) and a product is
// the six bf16 MFMA products hh, hm, mh, hl, lh, mm on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (dropped: ml, lm, ll,
// <= 2^-23 relative).  hh has an accumulator of its own, which so takes one rounding per 16 k; the five small products share a second.
//
// Operand maps of the 32x32x16 instruction: lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r],
// j = 0..7; C / D as in sw_gemm_kernel.  So a lane's eight k are CONTIGUOUS in both LDS tiles ([plane][row or column][k], pitch 40 bf16
// = 80 B: the 16-byte reads of 16 consecutive rows fall into distinct banks) and one ds_read_b128 fetches an operand.
//   weights      split once at pack time into three bf16 planes [plane][N][Kp], K-major per output column, Kp = K rounded up to 16 and
//                zero filled; staged as 16-byte copies.
//   activations  loaded as fp32 (four consecutive k of one row per thread: one 16-byte load where the addressing allows it, the
//                general per-element form otherwise -- cin % 4 != 0, NCHW input, the input affine, the K tail), split while staging.
// Rows m >= M, k >= K, columns n >= N and the zero padding of the conv are zeros in LDS; nothing is read or written outside them.
// No float atomics, a fixed summation order, and an output row depends on its own input row(s) only: an image's output is bitwise
// independent of its batch-mates, of B and of the run.  One limit: an fp32 value above bf16's largest finite value (the top 2^-8
// sliver under FLT_MAX) splits to inf, and its image's output is then non-finite.
//
// Everything is in an anonymous namespace: each including file compiles its own instance (as with sw_kernels.h).
#ifndef XSD_SW_GEMM_S3X_H
#define XSD_SW_GEMM_S3X_H
#include "sw_kernels.h"
#include "xsd_split.h"

namespace {

typedef __bf16 sx_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int sx_u32x4 __attribute__((ext_vector_type(4)));

constexpr int SXM = 128;        // rows per workgroup: wave w owns rows [32 w, 32 w + 32)
constexpr int SXN = 64;         // output columns per workgroup: two 32 x 32 column blocks per wave, two accumulators each
constexpr int SXK = 32;         // K per LDS round: two MFMA steps
constexpr int SXP = SXK + 8;    // LDS row pitch in bf16
// K rounds between flushes of the fp32 accumulators into doubles; 0 = plain fp32 accumulators
#ifndef SX_FLUSH
#define SX_FLUSH 0
#endif

inline int sx_kp(int K) { return (K + 15) / 16 * 16; }
inline long long sx_plane_elems(int N, int K) { return (long long)N * sx_kp(K); }      // one plane; a weight takes three

// [cout][cin][taps] as stored -> three bf16 planes [N = cout][Kp], k = tap * cin + ci, zeros for K <= k < Kp
__global__ __launch_bounds__(256) void sw_pack_s3x_kernel(const float* src, unsigned short* dst, int cout, int cin, int taps, int Kp)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long plane = (long long)cout * Kp;
    if (i >= plane) return;
    const int k = (int)(i % Kp), n = (int)(i / Kp);
    float v = 0.f;
    if (k < cin * taps) {
        const int t = k / cin, ci = k - t * cin;
        v = src[((long long)n * cin + ci) * taps + t];
    }
    xsd::split_f32x2 x;
    x[0] = v; x[1] = 0.f;
    unsigned int h, m, l;
    xsd::split3_pair(x, h, m, l);
    dst[i] = (unsigned short)(h & 0xffffu);
    dst[plane + i] = (unsigned short)(m & 0xffffu);
    dst[2 * plane + i] = (unsigned short)(l & 0xffffu);
}

__global__ __launch_bounds__(256) void sw_gemm_s3x_kernel(const GemmP P, const unsigned short* __restrict__ w3, const int Kp)
{
    __shared__ __attribute__((aligned(16))) unsigned short As[3][SXM][SXP];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[3][SXN][SXP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long M = (long long)P.B * P.HW;
    const long long m0 = (long long)blockIdx.x * SXM;
    const int n0 = blockIdx.y * SXN;

    // A: this thread stages k = k0 + 4 kq .. + 3 of the rows (tid >> 3) + 32 i
    const int kq = tid & 7;
    long long rbase[4];
    int ry[4], rx[4];
    bool rok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long m = m0 + (tid >> 3) + 32 * i;
        rok[i] = m < M;
        const long long b = rok[i] ? m / P.HW : 0, p = rok[i] ? m - b * P.HW : 0;
        rbase[i] = b * P.abs + (P.amode == A_TOK ? p * P.aps : 0);
        ry[i] = P.amode == A_CONV3 ? (int)(p / P.W) : 0;
        rx[i] = P.amode == A_CONV3 ? (int)(p - (long long)ry[i] * P.W) : 0;
    }
    // four consecutive k are four consecutive, 16-byte aligned floats of one tap (workgroup-uniform)
    const bool vec = P.acs == 1 && !P.isub && (P.aps & 3) == 0 && (P.abs & 3) == 0 && (P.cin & 3) == 0 &&
                     (reinterpret_cast<unsigned long long>(P.a) & 15) == 0;
    // B: column n0 + (tid >> 2), k = k0 + 8 (tid & 3) .. + 7 of each plane
    const int bn = n0 + (tid >> 2), bk = 8 * (tid & 3);
    const long long plane = (long long)P.N * Kp;
    const unsigned short* bsrc = w3 + (long long)(bn < P.N ? bn : 0) * Kp + bk;

    xsd::split_f32x4 av[4];
    sx_u32x4 bv[3];
    auto load = [&](int k0) {
        const int k = k0 + 4 * kq;
        if (P.amode == A_TOK) {
            if (vec && k + 4 <= P.K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    xsd::split_f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (rok[i]) v = *reinterpret_cast<const xsd::split_f32x4*>(P.a + rbase[i] + k);
                    av[i] = v;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[i][e] = (rok[i] && k + e < P.K) ? P.a[rbase[i] + (long long)(k + e) * P.acs] : 0.f;
            }
        } else if (vec) {
            const bool kok = k < P.K;                     // K = 9 cin is a multiple of 4 here: the group is inside K or outside
            const int tap = kok ? k / P.cin : 0, ci = kok ? k - tap * P.cin : 0;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int yy = ry[i] + dy, xx = rx[i] + dx;
                xsd::split_f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (rok[i] && kok && yy >= 0 && yy < P.H && xx >= 0 && xx < P.W)
                    v = *reinterpret_cast<const xsd::split_f32x4*>(P.a + rbase[i] + ci + SW_GEMM_EXT_SRC(yy, xx) * P.aps);
                av[i] = v;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {                 // a group of four k may straddle two taps: each k on its own
                const int ke = k + e;
                const bool kok = ke < P.K;
                const int tap = kok ? ke / P.cin : 0, ci = kok ? ke - tap * P.cin : 0;
                const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                const float sub = (P.isub && kok) ? P.isub[ci] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int yy = ry[i] + dy, xx = rx[i] + dx;
                    float v = 0.f;
                    if (rok[i] && kok && yy >= 0 && yy < P.H && xx >= 0 && xx < P.W) {
                        v = P.a[rbase[i] + (long long)ci * P.acs + SW_GEMM_EXT_SRC(yy, xx) * P.aps];
                        if (P.isub) v = (v - sub) * P.imul;
                    }
                    av[i][e] = v;
                }
            }
        }
        const bool bok = bn < P.N && k0 + bk < Kp;        // Kp is a multiple of 16, bk of 8: the eight k are inside Kp or outside
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            sx_u32x4 v = {0u, 0u, 0u, 0u};
            if (bok) v = *reinterpret_cast<const sx_u32x4*>(bsrc + pl * plane + k0);
            bv[pl] = v;
        }
    };

    f32x16 hh[2], sm[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int v = 0; v < 16; ++v) { hh[c][v] = 0.f; sm[c][v] = 0.f; }
#if SX_FLUSH
    double dd[2][16];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int v = 0; v < 16; ++v) dd[c][v] = 0.0;
    int since = 0;
#endif
    const int i32 = lane & 31, h2 = lane >> 5;
    load(0);
    for (int k0 = 0; k0 < P.K; k0 += SXK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xsd::split_u32x2 hi, mid, lo;
            xsd::split3_f32x4(av[i], hi, mid, lo);
            const int row = (tid >> 3) + 32 * i;
            *reinterpret_cast<xsd::split_u32x2*>(&As[0][row][4 * kq]) = hi;
            *reinterpret_cast<xsd::split_u32x2*>(&As[1][row][4 * kq]) = mid;
            *reinterpret_cast<xsd::split_u32x2*>(&As[2][row][4 * kq]) = lo;
        }
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<sx_u32x4*>(&Bs[pl][tid >> 2][bk]) = bv[pl];
        __syncthreads();
        if (k0 + SXK < P.K) load(k0 + SXK);
#pragma unroll
        for (int s = 0; s < SXK / 16; ++s) {
            if (k0 + 16 * s >= P.K) break;                // workgroup-uniform
            sx_bf16x8 a[3], b[2][3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                a[pl] = *reinterpret_cast<const sx_bf16x8*>(&As[pl][32 * wave + i32][16 * s + 8 * h2]);
                b[0][pl] = *reinterpret_cast<const sx_bf16x8*>(&Bs[pl][i32][16 * s + 8 * h2]);
                b[1][pl] = *reinterpret_cast<const sx_bf16x8*>(&Bs[pl][32 + i32][16 * s + 8 * h2]);
            }
            // the two column blocks alternate, so that no MFMA waits for the one just issued
#define SX_MM(acc, x, y)                                                                          \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[x], b[0][y], acc[0], 0, 0, 0);             \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[x], b[1][y], acc[1], 0, 0, 0);
            SX_MM(sm, 0, 2)     // hl
            SX_MM(sm, 2, 0)     // lh
            SX_MM(sm, 1, 1)     // mm
            SX_MM(hh, 0, 0)     // hh
            SX_MM(sm, 0, 1)     // hm
            SX_MM(sm, 1, 0)     // mh
#undef SX_MM
        }
#if SX_FLUSH
        if (++since == SX_FLUSH) {
            since = 0;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    dd[c][v] += (double)hh[c][v] + (double)sm[c][v];
                    hh[c][v] = 0.f; sm[c][v] = 0.f;
                }
        }
#endif
    }
    // accumulator register v of lane l: row 32 wave + 8 (v / 4) + 4 (l / 32) + v % 4, column 32 c + l % 32.  The epilogue is
    // sw_gemm_kernel's, statement for statement.
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n = n0 + 32 * c + i32;
        if (n >= P.N) continue;
        const float bn_ = P.bias ? P.bias[n] : 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long long m = m0 + 32 * wave + 8 * (v >> 2) + 4 * h2 + (v & 3);
            if (m >= M) continue;
#if SX_FLUSH
            float x = (float)(dd[c][v] + ((double)hh[c][v] + (double)sm[c][v])) + bn_;
#else
            float x = (hh[c][v] + sm[c][v]) + bn_;
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

hipError_t pack_s3x(hipStream_t s, const float* src, unsigned short* dst, int cout, int cin, int taps)
{
    const int Kp = sx_kp(cin * taps);
    const long long n = (long long)cout * Kp;
    hipLaunchKernelGGL(sw_pack_s3x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, cout, cin, taps, Kp);
    return hipGetLastError();
}

// p.w is not read: the weights are the planes at w3
hipError_t gemm_s3x(hipStream_t s, const GemmP& p, const unsigned short* w3)
{
    const long long M = (long long)p.B * p.HW;
    dim3 grid((unsigned)((M + SXM - 1) / SXM), (unsigned)((p.N + SXN - 1) / SXN));
    hipLaunchKernelGGL(sw_gemm_s3x_kernel, grid, dim3(256), 0, s, p, w3, sx_kp(p.K));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// host side: the math mode of an engine
// ---------------------------------------------------------------------------------------------------------------
// every gemm of a forward: the engine's mode decides the kernel; p.w names the weight by its fp32 packed copy
hipError_t gemm(hipStream_t s, const SwBase* r, const GemmP& p)
{
    if (r->math != 3) return gemm(s, p);
    const long long t = p.w - r->wt;
    auto it = std::lower_bound(r->lins.begin(), r->lins.end(), t, [](const Lin* l, long long v) { return l->t < v; });
    if (it == r->lins.end() || (*it)->t != t || !r->wt3) return hipErrorInvalidValue;
    return gemm_s3x(s, p, r->wt3 + (*it)->t3);
}

int pack_weights_s3x(SwBase* r, const char* net, hipStream_t s)
{
    for (const Lin* p : r->lins) {
        hipError_t e = pack_s3x(s, r->params + p->w, r->wt3 + p->t3, p->cout, p->cin, p->taps);
        if (e) return rfail(XSD_ERR_HIP, "%s weight packing (bf16x6): %s", net, hipGetErrorString(e));
    }
    r->packed3 = true;
    return XSD_OK;
}

// before a forward: in bf16x6 the planes exist and follow the last pack_weights (made here when the mode was set after it)
int ready_math(SwBase* r, const char* net, hipStream_t s)
{
    if (r->math != 3 || r->packed3) return XSD_OK;
    if (!r->wt3) {
        long long n = 0;
        for (Lin* p : r->lins) p->t3 = add(n, 3 * sx_plane_elems(p->cout, p->cin * p->taps));
        if (xsd::dev_alloc((void**)&r->wt3, sizeof(unsigned short) * std::max(8ll, n)) != hipSuccess) {
            (void)hipGetLastError();
            r->wt3 = nullptr;
            return rfail(XSD_ERR_NOMEM, "%s: allocation of the bf16x6 weight planes failed", net);
        }
    }
    return pack_weights_s3x(r, net, s);
}

int set_math(SwBase* r, const char* net, int mode)
{
    if (!r) return rfail(XSD_ERR_ARG, "null argument");
    if (mode == 4)
        return rfail(XSD_ERR_ARG, "%s: math mode f16x3 is not supported: its fp16 terms need a per-tensor scale (max |x|) that these kernels do not "
                     "publish; the math modes are fp32 and bf16x6", net);
    if (mode != 0 && mode != 3) return rfail(XSD_ERR_ARG, "%s: unknown math mode %d; the math modes are fp32 (0) and bf16x6 (3)", net, mode);
    r->math = mode;
    return XSD_OK;
}

// The GEMM on its own (tests): see include/xsd.h, xsd_sw_test_gemm.  With up2 (conv3 only, SW_GEMM_EXT) the conv runs over the nearest-2x
// upsampling of the H x W input: 4 B H W output rows.
int test_gemm(const float* dev_a, const float* dev_w, const float* dev_bias, float* dev_y, int conv3, int B, int H, int W, int cin, int N,
              long long ldy, int act, float slope, int math, hipStream_t s, bool up2 = false)
{
    if (!dev_a || !dev_w || !dev_y) return rfail(XSD_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1 || cin < 1 || N < 1 || ldy < N || (long long)B * H * W * (up2 ? 4 : 1) > (1ll << 28) || cin > 65536 || N > 65536)
        return rfail(XSD_ERR_ARG, "GEMM test: bad shape");
    if (act < ACT_NONE || act > ACT_LRELU) return rfail(XSD_ERR_ARG, "GEMM test: activation %d (0 none, 1 GELU, 2 LeakyReLU)", act);
    if (math != 0 && math != 3) return rfail(XSD_ERR_ARG, "GEMM test: the math modes are fp32 (0) and bf16x6 (3)");
    const int taps = conv3 ? 9 : 1, K = cin * taps;
    const long long wn = (long long)N * K;
    const size_t bytes = math == 3 ? sizeof(unsigned short) * (size_t)(3 * sx_plane_elems(N, K)) : sizeof(float) * (size_t)wn;
    void* wp = nullptr;
    if (xsd::dev_alloc(&wp, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "GEMM test: allocation failed");
    }
    hipError_t e;
    if (math == 3) {
        e = pack_s3x(s, dev_w, (unsigned short*)wp, N, cin, taps);
    } else {
        hipLaunchKernelGGL(sw_pack_kernel, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, s, dev_w, (float*)wp, N, cin, taps);
        e = hipGetLastError();
    }
    if (!e) {
        const long long rows = (long long)B * H * W;
        GemmP p = up2   ? gp_conv_up2(dev_a, B, H, W, cin, (const float*)wp, N, dev_bias, dev_y, ldy)
                : conv3 ? gp_conv(dev_a, B, H, W, cin, (const float*)wp, N, dev_bias, dev_y, ldy)
                        : gp_tok(dev_a, rows, cin, cin, (const float*)wp, N, dev_bias, dev_y, ldy);
        p.act = act; p.slope = slope;
        e = math == 3 ? gemm_s3x(s, p, (const unsigned short*)wp) : gemm(s, p);
    }
    hipStreamSynchronize(s);
    xsd::dev_free(wp);
    if (e) return rfail(XSD_ERR_HIP, "GEMM test: %s", hipGetErrorString(e));
    return XSD_OK;
}

// One launch described as the forwards describe theirs (tests): see include/xsd.h, xsd_sw_gemm_view.  GemmP comes from gp_tok / gp_conv /
// gp_conv_up2 plus the field assignments of head(), tail(), the SFB tail, out_nchw() and the SwinIR heads; the launch is theirs too.
// Host code only.  A file built without SW_GEMM_EXT refuses the fields its kernels do not read.
int test_gemm_view(const xsd_sw_gemm_view* v, hipStream_t s)
{
    if (!v) return rfail(XSD_ERR_ARG, "GEMM view test: the view is null");
    if (!v->a) return rfail(XSD_ERR_ARG, "GEMM view test: a is null");
    if (!v->w) return rfail(XSD_ERR_ARG, "GEMM view test: w is null");
    if (!v->y) return rfail(XSD_ERR_ARG, "GEMM view test: y is null");
    const bool conv = v->conv3 != 0, up2 = v->up2 != 0;
    const int B = v->B, H = v->H, W = v->W, cin = v->cin, N = v->N;
    if (B < 1 || H < 1 || W < 1 || cin < 1 || N < 1 || cin > 65536 || N > 65536 || H > (1 << 14) || W > (1 << 14))
        return rfail(XSD_ERR_ARG, "GEMM view test: bad shape B %d, H %d, W %d, cin %d, N %d", B, H, W, cin, N);
#if !SW_GEMM_EXT
    if (v->rnchw || v->cH || v->cW || v->up2 || v->omode == O_SHUFFLE_NCHW)
        return rfail(XSD_ERR_ARG, "GEMM view test: rnchw, cH, cW, up2 and omode 3 belong to xsd_swinir_test_gemm_view (this instance of the "
                     "kernel is built without them)");
#endif
    const int oH = up2 ? 2 * H : H, oW = up2 ? 2 * W : W;
    const long long rows = (long long)B * oH * oW;
    if (rows > (1ll << 28)) return rfail(XSD_ERR_ARG, "GEMM view test: %lld rows are too many", rows);
    if (v->act < ACT_NONE || v->act > ACT_LRELU) return rfail(XSD_ERR_ARG, "GEMM view test: act %d (0 none, 1 GELU, 2 LeakyReLU)", v->act);
    if (v->math != 0 && v->math != 3) return rfail(XSD_ERR_ARG, "GEMM view test: math %d; the math modes are fp32 (0) and bf16x6 (3)", v->math);
    if (!conv && (v->a_nchw || v->imean || up2 || v->rnchw || v->omode != O_TOK))
        return rfail(XSD_ERR_ARG, "GEMM view test: a_nchw, imean, up2, rnchw and omode %d need conv3 (token rows have no image)", v->omode);
    if (v->a_nchw && up2) return rfail(XSD_ERR_ARG, "GEMM view test: a_nchw with up2 is a form no forward launches");
    if (!v->a_nchw && (conv ? v->lda != cin : v->lda < cin))
        return rfail(XSD_ERR_ARG, "GEMM view test: lda %lld (token rows: at least cin = %d; conv3: exactly cin)", (long long)v->lda, cin);
    if (v->res && !conv && v->rbs != 0) return rfail(XSD_ERR_ARG, "GEMM view test: rbs %lld on token rows, which are one image", (long long)v->rbs);
    if (v->res && (v->rbs < 0 || v->rps < 0)) return rfail(XSD_ERR_ARG, "GEMM view test: negative rbs or rps");
    if (v->cH < 0 || v->cW < 0 || (v->cH == 0) != (v->cW == 0)) return rfail(XSD_ERR_ARG, "GEMM view test: cH %d and cW %d (both or neither)", v->cH, v->cW);
    const int r = v->r;
    switch (v->omode) {
    case O_TOK:
        if (v->ldy < N) return rfail(XSD_ERR_ARG, "GEMM view test: ldy %lld is less than N = %d", (long long)v->ldy, N);
        if (v->cH) return rfail(XSD_ERR_ARG, "GEMM view test: cH and cW go with omode 2 or 3");
        break;
    case O_SHUFFLE:
    case O_SHUFFLE_NCHW:
        if (r < 1 || r > 8 || N % (r * r)) return rfail(XSD_ERR_ARG, "GEMM view test: N = %d is no multiple of r^2 (r = %d, 1..8)", N, r);
        if (v->omode == O_SHUFFLE && v->cH) return rfail(XSD_ERR_ARG, "GEMM view test: cH and cW go with omode 2 or 3");
        if (v->omode == O_SHUFFLE_NCHW && !v->cH) return rfail(XSD_ERR_ARG, "GEMM view test: omode 3 needs cH and cW");
        if (v->cH > r * oH || v->cW > r * oW)
            return rfail(XSD_ERR_ARG, "GEMM view test: the crop cH %d x cW %d is larger than the %d x %d result", v->cH, v->cW, r * oH, r * oW);
        break;
    case O_NCHW:
        if (v->cH > oH || v->cW > oW)
            return rfail(XSD_ERR_ARG, "GEMM view test: the crop cH %d x cW %d is larger than the %d x %d result", v->cH, v->cW, oH, oW);
        break;
    default:
        return rfail(XSD_ERR_ARG, "GEMM view test: omode %d (0 token-major, 1 PixelShuffle, 2 NCHW, 3 PixelShuffle into NCHW)", v->omode);
    }
    if (v->omode == O_NCHW || v->omode == O_SHUFFLE_NCHW) {
        if (!v->omean) return rfail(XSD_ERR_ARG, "GEMM view test: omean is null");
        if (!(v->orange > 0)) return rfail(XSD_ERR_ARG, "GEMM view test: orange must be positive");
    }
    const int taps = conv ? 9 : 1, K = cin * taps;
    const long long wn = (long long)N * K;
    const size_t bytes = v->math == 3 ? sizeof(unsigned short) * (size_t)(3 * sx_plane_elems(N, K)) : sizeof(float) * (size_t)wn;
    void* wp = nullptr;
    if (xsd::dev_alloc(&wp, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return rfail(XSD_ERR_NOMEM, "GEMM view test: allocation failed");
    }
    hipError_t e;
    if (v->math == 3) {
        e = pack_s3x(s, v->w, (unsigned short*)wp, N, cin, taps);
    } else {
        hipLaunchKernelGGL(sw_pack_kernel, dim3((unsigned)((wn + 255) / 256)), dim3(256), 0, s, v->w, (float*)wp, N, cin, taps);
        e = hipGetLastError();
    }
    if (!e) {
        const long long ldy = v->omode == O_TOK ? v->ldy : 0, oHW = (long long)oH * oW;
        GemmP p = up2    ? gp_conv_up2(v->a, B, H, W, cin, (const float*)wp, N, v->bias, v->y, ldy)
                  : conv ? gp_conv(v->a, B, H, W, cin, (const float*)wp, N, v->bias, v->y, ldy)
                         : gp_tok(v->a, rows, cin, v->lda, (const float*)wp, N, v->bias, v->y, ldy);
        if (v->a_nchw) { p.acs = (long long)H * W; p.aps = 1; }                      // head()
        if (v->imean) { p.isub = v->imean; p.imul = v->irange; }
        p.act = v->act; p.slope = v->slope;
        if (v->res) { p.res = v->res; p.rbs = v->rbs; p.rps = v->rps; p.rnchw = v->rnchw; }
        if (v->omode == O_SHUFFLE) {                                                  // tail()
            p.omode = O_SHUFFLE; p.r = r; p.ybs = oHW * N; p.yps = N / (r * r);
        } else if (v->omode == O_NCHW) {                                              // tail(), out_nchw()
            p.omode = O_NCHW; p.ybs = N * oHW; p.omean = v->omean; p.orange = v->orange;
            if (v->cW) { p.cH = v->cH; p.cW = v->cW; p.ybs = (long long)N * v->cH * v->cW; }
        } else if (v->omode == O_SHUFFLE_NCHW) {                                      // UpsampleOneStep in swinir.hip
            p.omode = O_SHUFFLE_NCHW; p.r = r; p.cH = v->cH; p.cW = v->cW; p.ybs = (long long)(N / (r * r)) * v->cH * v->cW;
            p.omean = v->omean; p.orange = v->orange;
        }
        e = v->math == 3 ? gemm_s3x(s, p, (const unsigned short*)wp) : gemm(s, p);
    }
    hipStreamSynchronize(s);
    xsd::dev_free(wp);
    if (e) return rfail(XSD_ERR_HIP, "GEMM view test: %s", hipGetErrorString(e));
    return XSD_OK;
}

} // namespace

#endif /* XSD_SW_GEMM_S3X_H */
