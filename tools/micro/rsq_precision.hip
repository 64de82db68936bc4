// How accurate are v_rsq_f64 and v_rcp_f64, after the two Newton steps the kernels used to take, and after the one
// higher-order step they take now (rsqrt_pivot: third order, rcp_refined: second order)?  One run, the same arguments
// for every form; exits non-zero when a one-step form is worse than the two-step form by more than an ulp.
// hipcc --offload-arch=gfx950 -O3 tools/micro/rsq_precision.hip -o tools/micro/rsq_precision && tools/micro/rsq_precision
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <vector>
constexpr int NF = 8;
__global__ void k(const double *d, double *o, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = d[i];
    // ---- 1 / sqrt(x)
    double y0 = __builtin_amdgcn_rsq(x);
    double h = 0.5 * x;
    double y1 = y0 * fma(-h * y0, y0, 1.5);
    double y2 = y1 * fma(-h * y1, y1, 1.5);
    // one step, residual form: e = 1 - x y0^2 (fma), y = y0 + y0 * e / 2
    double e = fma(-x * y0, y0, 1.0);
    double y1r = fma(0.5 * y0, e, y0);
    // one third-order step (rsqrt_pivot): y0 (1 + r / 2 + 3 r^2 / 8)
    double t = x * y0, r = fma(-t, y0, 1.0);
    double p = fma(0.375, r, 0.5), yr = y0 * r;
    double y3 = fma(yr, p, y0);
    // ---- 1 / x
    double r0 = __builtin_amdgcn_rcp(x);
    double r1 = fma(fma(-x, r0, 1.0), r0, r0);
    double r2 = fma(fma(-x, r1, 1.0), r1, r1);
    // one second-order step (rcp_refined): r0 (1 + e + e^2)
    double er = fma(-x, r0, 1.0);
    double r3 = fma(fma(er, er, er), r0, r0);
    double *oo = o + (size_t)NF * i;
    oo[0] = y0; oo[1] = y1; oo[2] = y2; oo[3] = y1r; oo[4] = y3; oo[5] = r0; oo[6] = r2; oo[7] = r3;
}
// arguments exp((u - 1/2) * span), u uniform: span 40 is e^-20 .. e^20, span 1380 is 1e-300 .. 1e+300 (every argument,
// intermediate and result still a normal number)
static bool sweep(double span, const char *what)
{
    const int n = 1 << 20;
    std::vector<double> h(n), o((size_t)NF * n);
    unsigned long long s = 88172645463325252ull;
    for (int i = 0; i < n; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; double u = (s >> 11) * (1.0 / 9007199254740992.0); h[i] = std::exp((u - 0.5) * span); }
    double *dd, *dout;
    if (hipMalloc(&dd, n * 8) != hipSuccess || hipMalloc(&dout, (size_t)NF * n * 8) != hipSuccess) { printf("hipMalloc failed\n"); return false; }
    if (hipMemcpy(dd, h.data(), n * 8, hipMemcpyHostToDevice) != hipSuccess) { printf("copy failed\n"); return false; }
    hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, dd, dout, n);
    if (hipMemcpy(o.data(), dout, (size_t)NF * n * 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel or copy failed\n"); return false; }
    (void)hipFree(dd); (void)hipFree(dout);
    double m[NF] = {0};
    for (int i = 0; i < n; ++i) {
        const long double rq = 1.0L / sqrtl((long double)h[i]), rc = 1.0L / (long double)h[i];
        for (int q = 0; q < NF; ++q) {
            const long double ref = q < 5 ? rq : rc;
            double e = (double)fabsl(((long double)o[(size_t)NF * i + q] - ref) / ref);
            if (m[q] == m[q] && !(e <= m[q])) m[q] = e;          // (a NaN sticks)
        }
    }
    const double ulp = 1.1e-16;
    const bool ok_rsq = m[4] <= m[2] + ulp, ok_rcp = m[7] <= m[6] + ulp;
    printf("arguments %s (ulp = 1.1e-16), max relative error\n", what);
    printf("  1/sqrt(x): v_rsq_f64 %.3e, one Newton step %.3e, two steps %.3e, one step in residual form %.3e, one third-order step %.3e  [%s]\n",
           m[0], m[1], m[2], m[3], m[4], ok_rsq ? "ok: one third-order step <= two steps + 1 ulp" : "MISSED");
    printf("  1/x:       v_rcp_f64 %.3e, two Newton steps %.3e, one second-order step %.3e  [%s]\n",
           m[5], m[6], m[7], ok_rcp ? "ok: one second-order step <= two steps + 1 ulp" : "MISSED");
    return ok_rsq && ok_rcp;
}
int main()
{
    const bool a = sweep(40.0, "e^-20 .. e^+20"), b = sweep(1380.0, "1e-300 .. 1e+300");
    return a && b ? 0 : 1;
}
