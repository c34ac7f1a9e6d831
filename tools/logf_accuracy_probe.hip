// accuracy of the forward log stretch log(1000 v + 1) / log(1000) in several device forms, against the host's double
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
__global__ void k(const float* v, float* o, int n, int form)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = v[i], r;
    switch (form) {
    case 0: r = logf(1000.f * x + 1.f) / logf(1000.f); break;                       // the kernel's text
    case 1: r = logf(1000.f * x + 1.f); break;                                       // logf alone
    case 2: r = log1pf(1000.f * x) / logf(1000.f); break;
    case 3: r = (float)(log(fma(1000.0, (double)x, 1.0)) / log(1000.0)); break;      // double
    case 4: r = (float)log((double)(1000.f * x + 1.f)); break;                       // double log of the float argument, alone
    default: r = log2f(1000.f * x + 1.f); break;
    }
    o[i] = r;
}
int main()
{
    const int n = 6001;
    std::vector<float> v(n), o(n);
    for (int i = 0; i < n; ++i) v[i] = (float)(i / 6000.0);
    float *dv, *dout;
    if (hipMalloc(&dv, n * 4) != hipSuccess || hipMalloc(&dout, n * 4) != hipSuccess) return 1;
    hipMemcpy(dv, v.data(), n * 4, hipMemcpyHostToDevice);
    for (int form = 0; form < 6; ++form) {
        hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, dv, dout, n, form);
        if (hipMemcpy(o.data(), dout, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        double se = 0, mx = 0, su = 0, mu = 0;
        for (int i = 0; i < n; ++i) {
            const double a = 1000.0 * (double)v[i] + 1.0, af = (double)(1000.f * v[i] + 1.f);
            double ref = form == 0 || form == 2 || form == 3 ? log(a) / log(1000.0) : form == 5 ? log2(af) : log(af);
            double e = fabs((double)o[i] - ref);
            float rf = (float)ref; double ulp = fabs((double)nextafterf(rf, 2 * rf + 1) - rf);
            se += e * e; if (e > mx) mx = e; su += (e / ulp) * (e / ulp); if (e / ulp > mu) mu = e / ulp;
        }
        printf("form %d: rms %.3e max %.3e | rms %.3f ulp, max %.3f ulp\n", form, sqrt(se / n), mx, sqrt(su / n), mu);
    }
    return 0;
}
