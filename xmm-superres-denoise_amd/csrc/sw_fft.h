// sw_fft.h -- the FourierUnit's FFT passes (swinfir.py:14-61) in one place: the kernel, its launcher and the twiddle table of the fused
// SwinFIR forward (swinfir.hip), moved here unchanged so that a second translation unit can compile the same passes (DESIGN.md
// section 22: the differentiable rfftn / irfftn pair the SFB still lacks).  Included the way sw_kernels.h is: everything sits in an
// anonymous namespace and each including file compiles its own instance.
//
//   sw_fft_kernel    one pass of the FourierUnit's 2-D transform over lines of one axis: R2C along W, complex along H (forward and
//                    inverse), C2R along W.  Mixed-radix Stockham in LDS with radices 4, 2, 3, 5, 7, 11, 13 and twiddles from one
//                    table of the n-th roots of unity made in double.  The spectrum is stored as token rows
//                    [B][H][W/2+1][2 c + re/im]: the channel order of the reference's stack / permute / view, so the 1x1 conv over
//                    the spectrum is a plain token GEMM.  The butterflies are fp32 FMAs on the vector ALUs in a fixed order.
#ifndef XSD_SW_FFT_H
#define XSD_SW_FFT_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

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
// host side
// ---------------------------------------------------------------------------------------------------------------
// the factorisation the FFT passes use: 4s first, then the primes <= 13; false if another prime divides n
bool radices(int n, std::vector<int>& out)
{
    out.clear();
    while (n % 4 == 0) { out.push_back(4); n /= 4; }
    for (int p : {2, 3, 5, 7, 11, 13})
        while (n % p == 0) { out.push_back(p); n /= p; }
    return n == 1 && out.size() <= 16;
}


// the twiddle table of one (H, W): the H-th roots of unity, then the W-th, made in double and rounded to float
void fft_twiddles(int H, int W, float2* t)
{
    const double pi = std::acos(-1.0);
    for (int i = 0; i < H; ++i) t[i] = make_float2((float)std::cos(-2.0 * pi * i / H), (float)std::sin(-2.0 * pi * i / H));
    for (int i = 0; i < W; ++i) t[H + i] = make_float2((float)std::cos(-2.0 * pi * i / W), (float)std::sin(-2.0 * pi * i / W));
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

} // namespace

#endif /* XSD_SW_FFT_H */
