// slk_consistency.hpp -- Monte-Carlo consistency tools on the resident (mu, P) of a batch: the normalised estimation
// error squared (slk_nees) and Gaussian state draws x = mu [+] L n (slk_sample_states).  The reference has neither;
// both reuse its manifold operators (State.hpp:186-200: so3_boxminus / state_boxplus arithmetic of slk_math.hpp through
// the layout helpers of slk_kernels.hpp) and the factor the sigma points are drawn from (Eigen::LLT of Pk, lower).
// One 256-thread workgroup (4 waves) per filter, any state size; the packed factor and chol_blocked_mem's column panel
// live in a per-filter global workspace (consistency_ws), LDS holds only the 16 x 16 diagonal tile.  Both kernels read
// the LOWER triangle of P only (a lower-only covariance, slk_filter::upper_stale, needs no mirror) and write nothing
// but their outputs.
//   NEES: the bordered (n + 1) x (n + 1) matrix [[P_ss, .], [e^T, BIG]] is factored in one pass: its last row is
//         (L^-1 e)^T -- the forward substitution rides along in the panel / row-solve steps of the factorisation --
//         and NEES = |L^-1 e|^2.  BIG keeps the last pivot positive (it is never used).
//   draw: V = L [n_1 .. n_S] on fp64 MFMA (16 x 16 x 4, the tile loop of wide_mfma_k, C/D map as chol_blocked_mem: col = lane & 15 = sample,
//         row = (lane >> 4) + 4 * reg), 16 samples per pass, then x_s = mu [+] v_s per tangent index.
// A non-positive or NaN pivot of the (sub-)block gives that filter NaN outputs; no status bit is touched.
// The kernels are compiled in a translation unit of their own (slk_consistency.hip, SLK_CONSISTENCY_UNIT); slk_api.hip
// sees the workspace layout and the declarations only, so the device code of its kernels is what it was without them.
#pragma once
// (included after slk_kernels.hpp)

namespace slk {

// per-filter workspace (doubles): packed factor of n + 1 rows (NEES) or n (draws), the column panel, the error
// vector / one pass of draws
struct ConsWs { size_t Lp, panel, v, total; };
__host__ __device__ inline ConsWs consistency_ws(int n)
{
    ConsWs w;
    const size_t n1 = (size_t)n + 1, r16 = (n1 + 15) / 16 * 16;
    size_t o = 0;
    w.Lp = o;    o += n1 * (n1 + 1) / 2;
    w.panel = o; o += 17 * r16;
    w.v = o;     o += 16 * r16;                        // e (NEES) or V of 16 samples, column = sample, ld r16
    w.total = (o + 7) & ~(size_t)7;
    return w;
}

__global__ void nees_kernel(Lay L, const double *mean, const double *P, const double *truth, int t0, int n, double *nees,
                            double *err, double *wsbase);
__global__ void sample_states_kernel(Lay L, const double *mean, const double *P, const double *noise, int S, double *out,
                                     double *wsbase);

// Innovation consistency (slk_nis) and standard deviations (slk_get_sigma); slk_step_n_diag records both per step.
//   NIS:   SI [B][m * m + m] is what an emit-4 launch wrote (S column-major, then the innovation nu).  The bordered
//          (m + 1) x (m + 1) matrix [[S, .], [nu^T, BIG]] is factored as for the NEES: its last row is (Ls^-1 nu)^T, so
//          nis = |Ls^-1 nu|^2, and log det S = 2 sum log Ls_ii comes from the same pivots.  m <= STATS_ROWS_MAX: ONE wave
//          per filter (launched with 64 threads), chol_rows in registers, no workspace (the form of nees_rows_kernel);
//          above that four waves (256 threads) through chol_blocked_mem on the consistency_ws(m) workspace (the form of
//          nees_kernel).  Reads the lower triangle of S.  A non-positive or NaN pivot gives NaN in both outputs (an
//          emission that was skipped leaves the NaN the host filled SI with: the same answer).
//   sigma: sqrt of the diagonal of P on tangent indices [t0, t0 + n), one thread per number; a negative or NaN entry
//          gives NaN.  Nothing but the diagonal is read.
constexpr int STATS_ROWS_MAX = 30;     // m + 1 <= 31 rows of chol_rows
__global__ void innovation_stats_kernel(const double *SI, int m, double *nis, double *logdet, double *wsbase);
__global__ void sigma_kernel(const double *P, int B, int N, int t0, int n, double *sigma);

#ifdef SLK_CONSISTENCY_UNIT
// The SO(3) arithmetic takes its LEAF forms (the libm routes inlined): a call from these kernels to the out-of-line
// routes would change what the compiler infers for those functions, and with it the code of every existing kernel that
// calls them.  Same expressions, same results.
// component `comp` of the 3-vector a [-] b = log(b^-1 a) of SO(3) block `blk` (so3_boxminus)
__device__ __forceinline__ double so3_minus_comp(const Lay &L, const double *a, const double *b, int blk, int comp)
{
    double d0, d1, d2;
    so3_log<true>(qmul(qconj(ldq(b + so3_soff(L, blk))), ldq(a + so3_soff(L, blk))), d0, d1, d2);
    return comp == 0 ? d0 : (comp == 1 ? d1 : d2);
}

__device__ __forceinline__ double block_sum_256(double x, double *red, int tid)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += __shfl_down(x, s, 64);
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// nees [B]; err [B][n] or null.  truth [B][Nq]; e = (truth [-] mu) on tangent indices [t0, t0 + n).
__global__ __launch_bounds__(256) void nees_kernel(Lay L, const double *mean, const double *P, const double *truth,
                                                   int t0, int n, double *nees, double *err, double *wsbase)
{
    __shared__ __attribute__((aligned(16))) double cb[4 * 34 + 152];     // chol_blocked_mem: diagonal tile factor, pivots
    __shared__ double red[4];
    __shared__ int ish[1];
    const int bidx = blockIdx.x, tid = threadIdx.x, N = L.N, Nq = L.Nq;
    const ConsWs w = consistency_ws(n);
    double *ws = wsbase + (size_t)bidx * w.total;
    double *Lp = ws + w.Lp, *panel = ws + w.panel, *e = ws + w.v;
    const double *mu = mean + (size_t)bidx * Nq, *tr = truth + (size_t)bidx * Nq;
    const double *gP = P + (size_t)bidx * N * N;
    for (int i = tid; i < n; i += 256) {
        int blk = 0, comp = 0;
        const int s = t2s(L, t0 + i, blk, comp);
        const double v = s >= 0 ? tr[s] - mu[s] : so3_minus_comp(L, tr, mu, blk, comp);   // (a range may cut a block)
        e[i] = v;
        if (err) err[(size_t)bidx * n + i] = v;
    }
    __syncthreads();
    // init(i, j), i >= j: the sub-block's lower triangle, then the bordering row e^T and the corner
    const int fail = chol_blocked_mem<256>(Lp, n + 1, panel, cb, &ish[0], tid, [&](int i, int j) -> double {
        if (i < n) return gP[(t0 + i) + (size_t)(t0 + j) * N];
        return j < n ? e[j] : 0x1p1000;
    });
    double s2 = 0.0;
    for (int j = tid; j < n; j += 256) { const double y = Lp[pk(n + 1, n, j)]; s2 = fma(y, y, s2); }
    const double r = block_sum_256(s2, red, tid);
    if (tid == 0) nees[bidx] = fail >= 0 ? __builtin_nan("") : r;
}

// out [B][S][Nq] = mu [+] L noise[b][s], noise [B][S][N]
__global__ __launch_bounds__(256) void sample_states_kernel(Lay L, const double *mean, const double *P, const double *noise,
                                                            int S, double *out, double *wsbase)
{
    __shared__ __attribute__((aligned(16))) double cb[4 * 34 + 152];
    __shared__ int ish[1];
    const int bidx = blockIdx.x, tid = threadIdx.x, N = L.N, Nq = L.Nq;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const ConsWs w = consistency_ws(N);
    double *ws = wsbase + (size_t)bidx * w.total;
    double *Lp = ws + w.Lp, *panel = ws + w.panel, *V = ws + w.v;
    const int ldv = (N + 16) / 16 * 16;                  // (w.v is sized for n + 1 rows)
    const double *mu = mean + (size_t)bidx * Nq, *gP = P + (size_t)bidx * N * N;
    const double *nz = noise + (size_t)bidx * S * N;
    double *ob = out + (size_t)bidx * S * Nq;
    const int fail = chol_blocked_mem<256>(Lp, N, panel, cb, &ish[0], tid,
                                           [&](int i, int j) { return gP[i + (size_t)j * N]; });
    if (fail >= 0) {
        for (size_t e = tid; e < (size_t)S * Nq; e += 256) ob[e] = __builtin_nan("");
        return;
    }
    const int nt = (N + 15) / 16;
    for (int s0 = 0; s0 < S; s0 += 16) {
        // V(:, 0..15) = L [n_{s0} .. n_{s0 + 15}]: row tile I over k < min(16 I + 16, N) (L is lower triangular)
        for (int I = wave; I < nt; I += 4) {
            const int row = 16 * I + c, smp = s0 + c;
            const int k1 = round_up(min(16 * I + 16, N), 4);
            auto fa = [&](int k) { return (row < N && k <= row) ? Lp[pk(N, row, k)] : 0.0; };
            auto fb = [&](int k) { return (smp < S && k < N) ? nz[(size_t)smp * N + k] : 0.0; };
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            int kk = 0;
            for (; kk + 16 <= k1; kk += 16) {            // (the k loop of wide_mfma_k: loads of four k-steps first)
                double av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { av[u] = fa(kk + 4 * u + g); bv[u] = fb(kk + 4 * u + g); }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
            }
            for (; kk < k1; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(kk + g), fb(kk + g), acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) V[(size_t)c * ldv + 16 * I + g + 4 * r] = acc[r];
        }
        __syncthreads();
        const int ns = min(16, S - s0);
        for (int e = tid; e < ns * N; e += 256) {
            const int t = e % N, sl = e / N;
            const double *v = V + (size_t)sl * ldv;
            double *o = ob + (size_t)(s0 + sl) * Nq;
            int blk = 0, comp = 0;
            const int s = t2s(L, t, blk, comp);
            if (s >= 0) {
                o[s] = mu[s] + v[t];
            } else if (comp == 0) {                      // q [+] w = q exp(w), the whole block once
                const int so = so3_soff(L, blk);
                stq(o + so, qmul(ldq(mu + so), so3_exp<true>(v[t], v[t + 1], v[t + 2])));
            }
        }
        __syncthreads();
    }
}

// nis [B], logdet [B] (either may be null) from SI [B][m * m + m]; grid B, 64 threads for m <= STATS_ROWS_MAX, else 256
__global__ __launch_bounds__(256) void innovation_stats_kernel(const double *SI, int m, double *nis, double *logdet,
                                                               double *wsbase)
{
    __shared__ __attribute__((aligned(16))) double cb[4 * 34 + 152];     // chol_blocked_mem: diagonal tile factor, pivots
    __shared__ double Lr[31 * 32 / 2];                                   // the one-wave form's packed factor
    __shared__ double red[4];
    __shared__ int ish[1];
    const int bidx = blockIdx.x, tid = threadIdx.x;
    const double *S = SI + (size_t)bidx * (m * m + m), *nu = S + m * m;
    // init(i, j), i >= j for the blocked form; chol_rows hands any (row, column): the lower triangle of S either way
    auto init = [&](int i, int j) -> double {
        if (i < m) return j < m ? S[max(i, j) + m * min(i, j)] : 0.0;
        return j < m ? nu[j] : 0x1p1000;
    };
    if (m <= STATS_ROWS_MAX) {
        const int fail = chol_rows<31>(Lr, m + 1, tid, init);
        double s2 = 0.0, ld = 0.0;
        for (int j = 0; j < m; ++j) {
            const double y = Lr[pk(m + 1, m, j)];
            s2 = fma(y, y, s2);
            ld += log(Lr[pk(m + 1, j, j)]);
        }
        if (tid == 0) {
            if (nis) nis[bidx] = fail >= 0 ? __builtin_nan("") : s2;
            if (logdet) logdet[bidx] = fail >= 0 ? __builtin_nan("") : 2.0 * ld;
        }
        return;
    }
    const ConsWs w = consistency_ws(m);
    double *ws = wsbase + (size_t)bidx * w.total;
    double *Lp = ws + w.Lp, *panel = ws + w.panel;
    const int fail = chol_blocked_mem<256>(Lp, m + 1, panel, cb, &ish[0], tid, init);
    double s2 = 0.0, ld = 0.0;
    for (int j = tid; j < m; j += 256) {
        const double y = Lp[pk(m + 1, m, j)];
        s2 = fma(y, y, s2);
        ld += fail >= 0 ? 0.0 : log(Lp[pk(m + 1, j, j)]);
    }
    const double r = block_sum_256(s2, red, tid);
    __syncthreads();                                                     // (red is reused)
    const double l = block_sum_256(ld, red, tid);
    if (tid == 0) {
        if (nis) nis[bidx] = fail >= 0 ? __builtin_nan("") : r;
        if (logdet) logdet[bidx] = fail >= 0 ? __builtin_nan("") : 2.0 * l;
    }
}

// sigma [B][n] = sqrt(P_b(t0 + i, t0 + i)); grid ceil(B n / 256), 256 threads
__global__ __launch_bounds__(256) void sigma_kernel(const double *P, int B, int N, int t0, int n, double *sigma)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * n) return;
    const size_t b = e / n;
    const int i = t0 + (int)(e - b * n);
    sigma[e] = sqrt(P[b * (size_t)N * N + (size_t)i * (N + 1)]);        // (negative or NaN: NaN)
}

#endif // SLK_CONSISTENCY_UNIT

} // namespace slk
