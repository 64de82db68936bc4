// slk_trajectory.hpp -- the NEES records of slk_step_n for ranges of n <= 30 tangent indices: one WAVE per filter, the
// bordered (n + 1) x (n + 1) matrix [[P_ss, .], [e^T, BIG]] of nees_kernel (slk_consistency.hpp) factored in registers by
// chol_rows (lane = row, n + 1 <= 31 rows); its last row is (L^-1 e)^T and NEES = |L^-1 e|^2.  Where nees_kernel runs four
// waves through the blocked factorisation with a global workspace, this is one wave and no workspace; the result agrees
// with slk_nees to rounding (1e-10 relative), NaN exactly where a pivot is non-positive or NaN.  Reads the lower triangle
// of P only.  Compiled in a translation unit of its own (slk_trajectory.hip, SLK_TRAJ_UNIT); slk_api.hip sees the
// declaration only, so the device code of its kernels is what it was without it.
#pragma once
// (included after slk_kernels.hpp)

namespace slk {

constexpr int NEES_ROWS_MAX = 30;      // n + 1 <= 31 rows of chol_rows

// nees [B] for truth [B][Nq] on tangent indices [t0, t0 + n), n <= NEES_ROWS_MAX; grid B, 64 threads
__global__ void nees_rows_kernel(Lay L, const double *mean, const double *P, const double *truth, int t0, int n, double *nees);

#ifdef SLK_TRAJ_UNIT
// component `comp` of the 3-vector a [-] b = log(b^-1 a) of SO(3) block `blk` (nees_kernel's so3_minus_comp: the LEAF
// form of the SO(3) logarithm, same expressions, same results)
__device__ __forceinline__ double rows_so3_minus_comp(const Lay &L, const double *a, const double *b, int blk, int comp)
{
    double d0, d1, d2;
    so3_log<true>(qmul(qconj(ldq(b + so3_soff(L, blk))), ldq(a + so3_soff(L, blk))), d0, d1, d2);
    return comp == 0 ? d0 : (comp == 1 ? d1 : d2);
}

__global__ __launch_bounds__(64) void nees_rows_kernel(Lay L, const double *mean, const double *P, const double *truth,
                                                       int t0, int n, double *nees)
{
    __shared__ double Lp[31 * 32 / 2], e[32];
    const int bidx = blockIdx.x, lane = threadIdx.x, N = L.N, Nq = L.Nq;
    const double *mu = mean + (size_t)bidx * Nq, *th = truth + (size_t)bidx * Nq;
    const double *gP = P + (size_t)bidx * N * N;
    if (lane < n) {
        int blk = 0, comp = 0;
        const int s = t2s(L, t0 + lane, blk, comp);
        e[lane] = s >= 0 ? th[s] - mu[s] : rows_so3_minus_comp(L, th, mu, blk, comp);   // (a range may cut a block)
    }
    wave_sync();
    const int fail = chol_rows<31>(Lp, n + 1, lane, [&](int i, int j) -> double {
        if (i < n) return j < n ? gP[(t0 + max(i, j)) + (size_t)(t0 + min(i, j)) * N] : 0.0;   // (lower triangle only)
        return j < n ? e[j] : 0x1p1000;
    });
    double s2 = 0.0;
    for (int j = 0; j < n; ++j) { const double y = Lp[pk(n + 1, n, j)]; s2 = fma(y, y, s2); }
    if (lane == 0) nees[bidx] = fail >= 0 ? __builtin_nan("") : s2;
}
#endif // SLK_TRAJ_UNIT

} // namespace slk
