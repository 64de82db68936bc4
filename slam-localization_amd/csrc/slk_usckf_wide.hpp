// slk_usckf_wide.hpp -- Usckf::update (reference src/filters/Usckf.hpp:246-308) for every call the LDS-resident
// usckf_kernel does not take: more than MAXM = 32 measurement rows at any state size, and any update-side call (update,
// emit 2, emit 4) at N = 36 + nfk + nfkl > 96.  The reference's measurement dimension is ukfom::dof<_Measurement> and its
// feature blocks are dynamic (State.hpp:529-593): nothing bounds m or N but memory.  One 256-thread workgroup (4 waves) per
// filter; every N- and m-sized array lives in a per-filter global workspace (wide_ws), LDS holds only the 16 x 16 diagonal
// tiles of the two factors.  Every tile is masked by the true N and m, so any m >= 1 works.  The products run on fp64 MFMA
// (16 x 16 x 4, C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg, as chol_blocked_mem):
//   L = chol(P), packed lower      chol_blocked_mem, reads the LOWER triangle of P only
//   emit 2                         the update sigma points X from L (pert / sigma_quat), nothing else
//   Z = h(X), 2N + 1 sigma points  measure_item / pert / sigma_quat; EXTERNAL reads Zext in place
//   S = 1/2 sum dZ_i dZ_i^T + R    SYRK on the 16 x 16 lower tiles, k = sigma index (padded to 4)
//   covXZ = 1/2 (W o L) dZ^T       dZ_j = Z_{2j+1} - Z_{2j+2}; k runs over the nonzero columns of the row tile only
//   G = chol(S), packed lower      chol_blocked_mem
//   K = covXZ S^-1                 two triangular solves against G in 16-column blocks: off-diagonal block updates on
//                                  MFMA, the diagonal block one thread per row
//   gate, delta = K nu, P -= covXZ K^T (lower tiles, both triangles written from one value), direct boxplus
// Status bits, outlier counts, the emit-4 output ([S column-major, innovation]) and the whole-vector gate as in
// usckf_kernel<NT, 256>.  P is read from its lower triangle only, so the lower-only covariance the N = 48 split predict
// leaves (slk_filter::upper_stale) needs no mirror first.
#pragma once
// (included at the end of slk_usckf.hpp, after slk_usckf_general.hpp)

namespace slk {

// per-filter workspace of usckf_update_wide_kernel (doubles); every per-row array is sized by m
struct WideWs { size_t Lp, Gp, Sm, Cxz, K, Z, panel, zbar, innov, wv, delta, wgt, total; };
__host__ __device__ inline WideWs wide_ws(int N, int m)
{
    WideWs w;
    const size_t S = 2 * (size_t)N + 1, nm = N > m ? N : m;
    size_t o = 0;
    w.Lp = o;    o += (size_t)N * (N + 1) / 2;
    w.Gp = o;    o += (size_t)m * (m + 1) / 2;
    w.Sm = o;    o += (size_t)m * m;
    w.Cxz = o;   o += (size_t)N * m;
    w.K = o;     o += (size_t)N * m;
    w.Z = o;     o += S * m;
    w.panel = o; o += 17 * ((nm + 15) / 16 * 16);          // chol_blocked_mem's column panel, for both factors
    w.zbar = o;  o += m;
    w.innov = o; o += m;
    w.wv = o;    o += m;
    w.delta = o; o += N;
    w.wgt = o;   o += 3 * (size_t)N;                        // atan-wrap factor per (rotation block, column)
    w.total = (o + 7) & ~(size_t)7;
    return w;
}

// X_i [-] mu of rotation block b along column j of the packed factor: MTK's log uses atan, a column longer than pi wraps
__device__ __forceinline__ double usckf_wrap_weight_pk(const double *Lp, int N, int t0, int j)
{
    const double v0 = Lz(Lp, N, t0, j), v1 = Lz(Lp, N, t0 + 1, j), v2 = Lz(Lp, N, t0 + 2, j);
    const double th = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    return (th >= 3.141592653589793) ? 2.0 * atan(tan(0.5 * th)) / th : 1.0;
}

// acc += sum_{k0 <= k < k1} A(c, k) B(k, c') over one 16 x 16 tile: fa(k) is this lane's A operand (row lane & 15),
// fb(k) its B operand (column lane & 15), both 0 past the true bound; k1 - k0 a multiple of 4.  Loads of four k-steps first.
template <class FA, class FB>
__device__ __forceinline__ d4 wide_mfma_k(d4 acc, int k0, int k1, int g, FA fa, FB fb)
{
    int kk = k0;
    for (; kk + 16 <= k1; kk += 16) {
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { av[u] = fa(kk + 4 * u + g); bv[u] = fb(kk + 4 * u + g); }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; kk < k1; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(kk + g), fb(kk + g), acc, 0, 0, 0);
    return acc;
}

// the diagonal 16 x 16 tile C of the packed factor G (m x m) into LDS: packed, then reciprocal pivots at [136 + b]
__device__ __forceinline__ void wide_diag_tile(const double *Gp, int m, int C, double *gd, int tid)
{
    const int c0 = 16 * C, nc = (m - c0 < 16) ? (m - c0) : 16;
    for (int e = tid; e < 256; e += 256) {
        const int i = e & 15, j = e >> 4;
        if (i >= j && i < nc) gd[pk(16, i, j)] = Gp[pk(m, c0 + i, c0 + j)];
        if (i == j) gd[136 + i] = (i < nc) ? 1.0 / Gp[pk(m, c0 + i, c0 + i)] : 0.0;
    }
}

// Usckf::update (:246-308) and its sigma points (emit 2), any N and m.  One 256-thread workgroup per filter.
__global__ __launch_bounds__(256) void usckf_update_wide_kernel(KArgs a)
{
    __shared__ __attribute__((aligned(16))) double cb[4 * 34 + 152];     // chol_blocked_mem: diagonal tile factor, pivots
    __shared__ __attribute__((aligned(16))) double gd[152];              // diagonal tile of G for the solves
    __shared__ int ish[4];
    const int bidx = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    Lay L = a.lay;
    L.kind = SLK_USCKF;
    const int N = L.N, Nq = L.Nq, m = a.m, S = 2 * N + 1;
    const int nt = (N + 15) / 16, mt = (m + 15) / 16;
    const WideWs w = wide_ws(N, m);
    double *ws = a.wsL + (size_t)bidx * w.total;
    double *Lp = ws + w.Lp, *Gp = ws + w.Gp, *Sm = ws + w.Sm, *Cxz = ws + w.Cxz, *K = ws + w.K, *Z = ws + w.Z;
    double *panel = ws + w.panel, *zbar = ws + w.zbar, *innov = ws + w.innov, *wv = ws + w.wv, *dlt = ws + w.delta;
    double *wgt = ws + w.wgt;
    double *mu = a.mean + (size_t)bidx * Nq;               // (read in place: written only after the last read)
    double *gP = a.P + (size_t)bidx * N * N;
    int status = 0;
    SLK_STAMP_NR(0);
    if (a.do_update && a.emit != 4 && tid == 0) a.outliers[bidx] = 0u;
    // ---- sigma points of the full state: Usckf.hpp:273 -> :532-598 (Eigen::LLT of Pk, lower triangle)
    const int fail = chol_blocked_mem<256>(Lp, N, panel, cb, &ish[0], tid,
                                           [&](int i, int j) { return gP[i + (size_t)j * N]; });
    SLK_STAMP_NR(1);
    if (fail >= 0) {
        status |= SLK_ST_LLT_FAIL;                          // the filter is left unchanged
    } else if (a.emit == 2) {
        double *X = a.Xout + (size_t)bidx * S * Nq;
        for (size_t e = tid; e < (size_t)S * N; e += 256) {
            const int t = (int)(e % N), i = (int)(e / N);
            int blk = 0, comp = 0;
            const int s = t2s(L, t, blk, comp);
            if (s >= 0) X[(size_t)i * Nq + s] = mu[s] + pert(Lp, N, nullptr, t, sig_of(i));
        }
        for (size_t e = tid; e < (size_t)S * 3; e += 256) {
            const int b = (int)(e % 3), i = (int)(e / 3);
            stq(X + (size_t)i * Nq + so3_soff(L, b), sigma_quat(L, mu, Lp, nullptr, b, sig_of(i)));
        }
    } else if (!pose_params_ok(a, L, a.mp ? a.mp + (size_t)bidx * a.mp_stride : nullptr)) {
        status |= SLK_ST_BAD_INDEX;                         // pose index out of 0..2: update skipped
    } else {
        const double *mp = a.mp ? a.mp + (size_t)bidx * a.mp_stride : nullptr;
        // Z = h(X) (:275-276): [2N + 1][m]
        const double *Zs = Z;
        if (a.mm == SLK_MODEL_EXTERNAL) {
            Zs = a.Zext + (size_t)bidx * S * m;
        } else {
            const int nf = measure_features(a.mm, m);
            for (size_t e = tid; e < (size_t)S * nf; e += 256) {
                const int f = (int)(e % nf), i = (int)(e / nf);
                measure_item(a, L, mp, mu, Lp, i, f, Z + (size_t)i * m);
            }
        }
        for (int e = tid; e < 3 * N; e += 256) {
            const int j = e % N, b = e / N;
            wgt[e] = usckf_wrap_weight_pk(Lp, N, so3_toff(L, b), j);
        }
        __syncthreads();
        SLK_STAMP_NR(2);
        // mean_z (:278), innovation (:290)
        for (int r = tid; r < m; r += 256) {
            double s = 0.0;
            for (int i = 0; i < S; ++i) s += Zs[(size_t)i * m + r];
            zbar[r] = s / (double)S;
            innov[r] = a.z[(size_t)bidx * m + r] - zbar[r];
        }
        __syncthreads();
        // S = cov(Z) + R (:280), the lower 16 x 16 tiles on the matrix cores, both triangles written from one value
        const double *R = a.R + (size_t)bidx * a.r_stride;
        const int S4 = (S + 3) & ~3;
        for (int T = wave; T < mt * (mt + 1) / 2; T += 4) {
            int I = 0;
            while ((I + 1) * (I + 2) / 2 <= T) ++I;
            const int J = T - I * (I + 1) / 2;
            const int ra = 16 * I + c, rb = 16 * J + c;
            const bool oka = ra < m, okb = rb < m;
            const double za = zbar[oka ? ra : 0], zb = zbar[okb ? rb : 0];
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            acc = wide_mfma_k(acc, 0, S4, g,
                [&](int k) { const bool in = oka && k < S; const double v = Zs[in ? (size_t)k * m + ra : 0]; return in ? v - za : 0.0; },
                [&](int k) { const bool in = okb && k < S; const double v = Zs[in ? (size_t)k * m + rb : 0]; return in ? v - zb : 0.0; });
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + g + 4 * r, col = 16 * J + c;
                if (row < m && col < m && row >= col) {
                    const double v = 0.5 * acc[r];
                    Sm[row + (size_t)col * m] = v + R[row + (size_t)col * m];
                    if (row != col) Sm[col + (size_t)row * m] = v + R[col + (size_t)row * m];
                }
            }
        }
        SLK_STAMP_NR(3);
        if (a.emit == 4) {
            __syncthreads();
            // innovation and its covariance for a caller-side significance test: Xout [B][m*m + m] = S (column-major),
            // innovation; nothing else happens
            double *o = a.Xout + (size_t)bidx * ((size_t)m * m + m);
            for (size_t e = tid; e < (size_t)m * m; e += 256) o[e] = Sm[e];
            for (int e = tid; e < m; e += 256) o[(size_t)m * m + e] = innov[e];
        } else {
            // covXZ = 1/2 sum (X_i [-] mu)(Z_i - mean_z)^T (:281 -> :691-712): the +- pairs of column j contribute
            // +- w L(:, j) (Z_{2j+1} - Z_{2j+2}), the mean_z terms cancel.  Row tile I: columns j <= 16 I + 15 only.
            for (int T = wave; T < nt * mt; T += 4) {
                const int I = T % nt, Jc = T / nt;
                const int t = 16 * I + c, rb = 16 * Jc + c;
                const bool okt = t < N, okb = rb < m;
                int blk = -1, comp = 0;
                const int s = okt ? t2s(L, t, blk, comp) : 0;
                const double *wrow = (s < 0) ? wgt + (size_t)blk * N : nullptr;
                const int kend = (16 * I + 16 < N) ? 16 * I + 16 : ((N + 3) & ~3);
                d4 acc = {0.0, 0.0, 0.0, 0.0};
                acc = wide_mfma_k(acc, 0, kend, g,
                    [&](int j) {
                        const bool in = okt && j <= t;
                        const double l = Lp[in ? pk(N, t, j) : 0], wj = (in && wrow) ? wrow[j] : 1.0;
                        return in ? wj * l : 0.0;
                    },
                    [&](int j) {
                        const bool in = okb && j < N;
                        const double z1 = Zs[in ? (size_t)(2 * j + 1) * m + rb : 0], z2 = Zs[in ? (size_t)(2 * j + 2) * m + rb : 0];
                        return in ? z1 - z2 : 0.0;
                    });
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * I + g + 4 * r, col = 16 * Jc + c;
                    if (row < N && col < m) Cxz[row + (size_t)N * col] = 0.5 * acc[r];
                }
            }
            __syncthreads();
            SLK_STAMP_NR(4);
            // S^-1 (:285-286): S = 1/2 dZ dZ^T + R is SPD for a valid R -> its Cholesky factor G (packed lower)
            const int sfail = chol_blocked_mem<256>(Gp, m, panel, cb, &ish[0], tid,
                                                    [&](int i, int j) { return Sm[i + (size_t)j * m]; });
            SLK_STAMP_NR(5);
            if (sfail >= 0) {
                status |= SLK_ST_SINGULAR;
            } else {
                // K = covXZ S^-1 (:288): Y G^T = covXZ (forward over column blocks), then K G = Y (backward), Y and K in K
                for (int C = 0; C < mt; ++C) {
                    const int c0 = 16 * C;
                    wide_diag_tile(Gp, m, C, gd, tid);
                    for (int I = wave; I < nt; I += 4) {     // block C of covXZ minus Y(:, 0:c0) G(c0 + ., 0:c0)^T
                        const int t = 16 * I + c, col = c0 + c;
                        const bool okt = t < N, okc = col < m;
                        d4 acc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * I + g + 4 * r;
                            acc[r] = (row < N && col < m) ? Cxz[row + (size_t)N * col] : 0.0;
                        }
                        acc = wide_mfma_k(acc, 0, c0, g,
                            [&](int p) { const double v = K[okt ? t + (size_t)N * p : 0]; return okt ? -v : 0.0; },
                            [&](int p) { const double v = Gp[okc ? pk(m, col, p) : 0]; return okc ? v : 0.0; });
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * I + g + 4 * r;
                            if (row < N && col < m) K[row + (size_t)N * col] = acc[r];
                        }
                    }
                    __syncthreads();
                    const int nc = (m - c0 < 16) ? (m - c0) : 16;
                    for (int t = tid; t < N; t += 256) {     // the diagonal block, one row per thread
                        int o = 0;                                  // (opaque: keeps the 136 tile loads in the loop
                        asm volatile("" : "+v"(o));                 // instead of hoisted into registers)
                        const double *gt = gd + o;
                        double x[16];
#pragma unroll
                        for (int b = 0; b < 16; ++b) {
                            x[b] = 0.0;
                            if (b < nc) {
                                double sum = K[t + (size_t)N * (c0 + b)];
#pragma unroll
                                for (int q = 0; q < b; ++q) sum -= x[q] * gt[pk(16, b, q)];
                                x[b] = sum * gt[136 + b];
                                K[t + (size_t)N * (c0 + b)] = x[b];
                            }
                        }
                    }
                    __syncthreads();
                }
                for (int C = mt - 1; C >= 0; --C) {
                    const int c0 = 16 * C;
                    wide_diag_tile(Gp, m, C, gd, tid);
                    const int k0 = c0 + 16, k1 = (m + 3) & ~3;
                    for (int I = wave; I < nt && k0 < m; I += 4) {     // block C of Y minus K(:, c0+16:m) G(c0+16:m, c0 + .)
                        const int t = 16 * I + c, col = c0 + c;
                        const bool okt = t < N, okc = col < m;
                        d4 acc;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * I + g + 4 * r;
                            acc[r] = (row < N && col < m) ? K[row + (size_t)N * col] : 0.0;
                        }
                        acc = wide_mfma_k(acc, k0, k1, g,
                            [&](int p) { const bool in = okt && p < m; const double v = K[in ? t + (size_t)N * p : 0]; return in ? -v : 0.0; },
                            [&](int p) { const bool in = okc && p < m; const double v = Gp[in ? pk(m, p, col) : 0]; return in ? v : 0.0; });
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * I + g + 4 * r;
                            if (row < N && col < m) K[row + (size_t)N * col] = acc[r];
                        }
                    }
                    __syncthreads();
                    const int nc = (m - c0 < 16) ? (m - c0) : 16;
                    for (int t = tid; t < N; t += 256) {
                        int o = 0;
                        asm volatile("" : "+v"(o));
                        const double *gt = gd + o;
                        double x[16];
#pragma unroll
                        for (int b = 15; b >= 0; --b) {
                            x[b] = 0.0;
                            if (b < nc) {
                                double sum = K[t + (size_t)N * (c0 + b)];
#pragma unroll
                                for (int q = b + 1; q < 16; ++q) sum -= (q < nc ? x[q] * gt[pk(16, q, b)] : 0.0);
                                x[b] = sum * gt[136 + b];
                                K[t + (size_t)N * (c0 + b)] = x[b];
                            }
                        }
                    }
                    __syncthreads();
                }
                SLK_STAMP_NR(6);
                if (tid == 0) {                                  // mahalanobis2 = |Ls^-1 innovation|^2 (:292)
                    bool ok = true;
                    if (a.gate > 9) {
                        ok = false;                              // Usckf.hpp:794-855: no table entry, default branch
                    } else if (a.gate > 0) {
                        double d2 = 0.0;
                        for (int r = 0; r < m; ++r) {
                            double sum = innov[r];
                            for (int p = 0; p < r; ++p) sum -= Gp[pk(m, r, p)] * wv[p];
                            wv[r] = sum / Gp[pk(m, r, r)];
                            d2 += wv[r] * wv[r];
                        }
                        const double thr[10] = {0, 3.84, 5.99, 7.81, 9.49, 11.07, 12.59, 14.07, 15.51, 16.92};
                        ok = d2 < thr[a.gate];
                    }
                    ish[1] = ok ? 1 : 0;
                }
                __syncthreads();
                if (!ish[1]) {
                    if (tid == 0) a.outliers[bidx] = 1u;
                    status |= SLK_ST_ALL_REJECTED;
                } else {
                    for (int t = tid; t < N; t += 256) {         // K * innovation (:299)
                        double sum = 0.0;
                        for (int r = 0; r < m; ++r) sum += K[t + (size_t)N * r] * innov[r];
                        dlt[t] = sum;
                    }
                    // Pk -= K S K^T (:296; K S = covXZ) on the lower 16 x 16 tiles: the lower triangle read, both
                    // triangles written from one value
                    const int m4 = (m + 3) & ~3;
                    for (int T = wave; T < nt * (nt + 1) / 2; T += 4) {
                        int I = 0;
                        while ((I + 1) * (I + 2) / 2 <= T) ++I;
                        const int J = T - I * (I + 1) / 2;
                        const int ra = 16 * I + c, rb = 16 * J + c;
                        const bool oka = ra < N, okb = rb < N;
                        d4 acc = {0.0, 0.0, 0.0, 0.0};
                        acc = wide_mfma_k(acc, 0, m4, g,
                            [&](int k) { const bool in = oka && k < m; const double v = Cxz[in ? ra + (size_t)N * k : 0]; return in ? v : 0.0; },
                            [&](int k) { const bool in = okb && k < m; const double v = K[in ? rb + (size_t)N * k : 0]; return in ? v : 0.0; });
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int i = 16 * I + g + 4 * r, j = 16 * J + c;
                            if (i < N && j < N && i >= j) {
                                const double v = gP[i + (size_t)j * N] - acc[r];
                                gP[i + (size_t)j * N] = v;
                                gP[j + (size_t)i * N] = v;
                            }
                        }
                    }
                    __syncthreads();
                    // mu_state = mu_state + state(K * innovation) (:299-301), the direct boxplus
                    for (int t = tid; t < N; t += 256) {
                        int blk = 0, comp = 0;
                        const int s = t2s(L, t, blk, comp);
                        if (s >= 0) mu[s] = mu[s] + dlt[t];
                    }
                    for (int b = tid; b < 3; b += 256) {
                        const int to = so3_toff(L, b), so = so3_soff(L, b);
                        stq(mu + so, qmul(ldq(mu + so), so3_exp(dlt[to], dlt[to + 1], dlt[to + 2])));
                    }
                }
            }
        }
    }
    SLK_STAMP_NR(7);
    if (tid == 0 && status) atomicOr(a.status + bidx, status);
}

} // namespace slk
