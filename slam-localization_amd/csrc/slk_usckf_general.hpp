// slk_usckf_general.hpp -- localization::Usckf (reference src/filters/Usckf.hpp) for states of ANY size: the shapes beyond
// the LDS-resident usckf_kernel (N = 36 + nfk + nfkl > 96; the two feature blocks are dynamic, State.hpp:529-593,
// Usckf.hpp:322-389).  The same model as msckf_update_general_kernel (slk_general.hpp): one workgroup per filter, every
// N-sized array in a per-filter global workspace (general_ws with the packed factor), plain loops in the reference's own
// order of operations -- no matrix cores, no LDS tiling.  A step is two launches:
//   usckf_predict_general_kernel (one wave): the 12-DOF prediction of statek_i (predict_phase), Fk = Pxy^T Pk_i^-1 (:154)
//     and the cross blocks (:154-235), streamed one column of P per lane -- nothing N-sized is staged;
//   usckf_update_general_kernel (256 threads): L = chol(P) -> Z = h(X) over the implicit sigma points -> mean_z, S, covXZ
//     (MTK's atan wrap of long rotation columns) -> chol(S) -> K = covXZ S^-1, the whole-vector chi-square gate -> P -= K S K^T
//     (both triangles from one value) and the direct boxplus of K * innovation (:246-308).
// Modes and status bits as in usckf_kernel<NT, 256>: emit 1 (predict sigma points) / 2 (update sigma points) / 4 (innovation
// and its covariance), registered models or Z / Y from the caller (SLK_MODEL_EXTERNAL).
#pragma once
// (included at the end of slk_usckf.hpp: uses the helpers of slk_kernels.hpp and slk_general.hpp)

namespace slk {

// Usckf::predict, Usckf.hpp:107-244, any N.  One wave per filter (at the residency of usckf_predict_kernel); the covariance
// stays in global memory.
__global__ __launch_bounds__(64, UPRED_WAVES) void usckf_predict_general_kernel(KArgs a)
{
    __shared__ __attribute__((aligned(16))) double sm[16 + 3 * 160 + 736 + 144];
    const int bidx = blockIdx.x, tid = threadIdx.x;
    const int N = a.lay.N, Nq = a.lay.Nq;
    double *mu = sm, *Pn = sm + 16, *Lblk = Pn + 160, *Pxy = Lblk + 160, *scr = Pxy + 160, *Fk = scr + 736;
    double *gmean = a.mean + (size_t)bidx * Nq;
    double *gP = a.P + (size_t)bidx * N * N;
    if (tid < 13) mu[tid] = gmean[26 + tid];
    __syncthreads();
    const int st = predict_phase<true>(a, bidx, tid, [&](int i, int j) { return gP[(24 + i) + (size_t)(24 + j) * N]; },
                                       Lblk, mu, Pn, scr, Pxy);
    if (st < 0) return;                              // sigma points emitted
    if (!(st & SLK_ST_LLT_FAIL)) {
        // Fk = Pxy^T * Pk_i^-1 (:154): Pk_i = L L^T, Pxy = L M (predict_phase hands out M), Fk^T = L^-T M
        if (tid < 12) {
            double x[12];                            // (every loop over it unrolled: registers, no scratch memory)
#pragma unroll
            for (int r = 11; r >= 0; --r) {
                double s = Pxy[r + 12 * tid];
#pragma unroll
                for (int p = r + 1; p < 12; ++p) s -= Lblk[pk(12, p, r)] * x[p];
                x[r] = s / Lblk[pk(12, r, r)];
            }
#pragma unroll
            for (int r = 0; r < 12; ++r) Fk[tid + 12 * r] = x[r];      // column tid of Fk^T = row tid of Fk
        }
        __syncthreads();
        // the cross blocks of state k+i, one column c of P per lane: its 12 old entries P(24 + p, c) are read from the lower
        // triangle (down column 24 + p for the features: coalesced over the lanes) into registers, the 12 new ones
        // (Fk * old)(r) go to both triangles -- rows against statek, statek_l and both feature blocks (:200-208, :221-232),
        // columns against statek / statek_l (:190-198) and feature rows (:227, :235) as their transposes.  No lane reads
        // an entry another lane writes.
        for (int c = tid; c < N; c += 64) {
            if (c >= 24 && c < 36) continue;
            double old[12];
#pragma unroll
            for (int p = 0; p < 12; ++p) old[p] = (c < 24) ? gP[(24 + p) + (size_t)c * N] : gP[c + (size_t)(24 + p) * N];
#pragma unroll 1
            for (int r = 0; r < 12; ++r) {          // (not unrolled: Fk stays in LDS instead of 144 registers hoisted out of the c loop)
                double s = 0.0;
#pragma unroll
                for (int p = 0; p < 12; ++p) s += Fk[r + 12 * p] * old[p];
                gP[(24 + r) + (size_t)c * N] = s;
                gP[c + (size_t)(24 + r) * N] = s;
            }
        }
        for (int e = tid; e < 144; e += 64) gP[(24 + e % 12) + (size_t)(24 + e / 12) * N] = Pn[e];
        if (tid < 13) gmean[26 + tid] = mu[tid];
    }
    if (tid == 0 && st) atomicOr(a.status + bidx, st);
}

// X_i [-] mu of rotation block b along column j of the factor: MTK's log uses atan, a column longer than pi wraps
__device__ __forceinline__ double usckf_wrap_weight(const double *Lm, int N, int t0, int j)
{
    const double v0 = j <= t0 ? Lm[t0 + (size_t)j * N] : 0.0, v1 = j <= t0 + 1 ? Lm[t0 + 1 + (size_t)j * N] : 0.0;
    const double v2 = j <= t0 + 2 ? Lm[t0 + 2 + (size_t)j * N] : 0.0;
    const double th = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    return (th >= 3.141592653589793) ? 2.0 * atan(tan(0.5 * th)) / th : 1.0;
}

// Usckf::update, Usckf.hpp:246-308 (generateSigmaPoints :532-598), any N.  One 256-thread workgroup per filter.
__global__ __launch_bounds__(256) void usckf_update_general_kernel(KArgs a)
{
    __shared__ int ish[64];
    const int bidx = blockIdx.x, tid = threadIdx.x;
    Lay L = a.lay;
    L.kind = SLK_USCKF;
    const int N = L.N, Nq = L.Nq, m = a.m, S = 2 * N + 1;
    const GenWs w = general_ws(N, Nq, 3, m > 0 ? m : 1, true);
    double *ws = a.wsL + (size_t)bidx * w.total;
    double *Lm = ws + w.L, *Lp = ws + w.Lp, *Z = ws + w.Z, *DZ = ws + w.DZ, *Cxz = ws + w.Cxz, *K = ws + w.K, *Sm = ws + w.Sm;
    double *G = ws + w.G, *zbar = ws + w.zbar, *innov = ws + w.innov, *dlt = ws + w.delta, *wv = ws + w.md, *wgt = ws + w.wgt;
    double *mu = a.mean + (size_t)bidx * Nq;               // (read in place: written only after the last read)
    double *gP = a.P + (size_t)bidx * N * N;
    int status = 0;
    if (a.do_update && a.emit != 4 && tid == 0) a.outliers[bidx] = 0u;
    for (size_t e = tid; e < (size_t)N * N; e += 256) Lm[e] = gP[e];       // (the factorisation reads the lower triangle only)
    __syncthreads();
    // ---- sigma points of the full state: Usckf.hpp:273 -> :532-598 (Eigen::LLT of Pk)
    const int fail = general_cholesky(Lm, N, tid, &ish[44]);
    if (fail >= 0) {
        status |= SLK_ST_LLT_FAIL;                          // the filter is left unchanged
    } else {
        // the packed copy of the factor the measurement models of the LDS kernels read (pert / sigma_quat / measure_item)
        for (size_t e = tid; e < (size_t)N * N; e += 256) {
            const int i = (int)(e % N), j = (int)(e / N);
            if (i >= j) Lp[pk(N, i, j)] = Lm[e];
        }
        __syncthreads();
        if (a.emit == 2) {
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
            status |= SLK_ST_BAD_INDEX;                     // pose index out of 0..2: update skipped
        } else {
            const double *mp = a.mp ? a.mp + (size_t)bidx * a.mp_stride : nullptr;
            // Z = h(X) (:275-276)
            if (a.mm == SLK_MODEL_EXTERNAL) {
                const double *Ze = a.Zext + (size_t)bidx * S * m;
                for (size_t e = tid; e < (size_t)S * m; e += 256) Z[e] = Ze[e];
            } else {
                const int nf = measure_features(a.mm, m);
                for (size_t e = tid; e < (size_t)S * nf; e += 256) {
                    const int f = (int)(e % nf), i = (int)(e / nf);
                    measure_item(a, L, mp, mu, Lp, i, f, Z + (size_t)i * m);
                }
            }
            for (int e = tid; e < 3 * N; e += 256) {
                const int j = e % N, b = e / N;
                wgt[e] = usckf_wrap_weight(Lm, N, so3_toff(L, b), j);
            }
            __syncthreads();
            // mean_z (:278), innovation (:290)
            for (int r = tid; r < m; r += 256) {
                double s = 0.0;
                for (int i = 0; i < S; ++i) s += Z[(size_t)i * m + r];
                zbar[r] = s / (double)S;
                innov[r] = a.z[(size_t)bidx * m + r] - zbar[r];
            }
            for (size_t e = tid; e < (size_t)N * m; e += 256) {
                const int r = (int)(e % m), j = (int)(e / m);
                DZ[e] = Z[(size_t)(2 * j + 1) * m + r] - Z[(size_t)(2 * j + 2) * m + r];
            }
            __syncthreads();
            // S = cov(Z) + R (:280); covXZ = 1/2 sum (X_i [-] mu)(Z_i - mean_z)^T (:281 -> :691-712): the +- pairs of column j
            // contribute +- w L(:, j) (Z_{2j+1} - Z_{2j+2}), the mean_z terms cancel
            const double *R = a.R + (size_t)bidx * a.r_stride;
            for (int e = tid; e < m * m; e += 256) {
                const int ra = e % m, rb = e / m;
                double s = 0.0;
                for (int i = 0; i < S; ++i) s += (Z[(size_t)i * m + ra] - zbar[ra]) * (Z[(size_t)i * m + rb] - zbar[rb]);
                Sm[e] = 0.5 * s + R[e];
            }
            for (size_t e = tid; e < (size_t)N * m; e += 256) {
                const int t = (int)(e % N), r = (int)(e / N);
                int blk = -1, comp = 0;
                const int s = t2s(L, t, blk, comp);
                double sum = 0.0;
                for (int j = 0; j <= t; ++j) sum += (s < 0 ? wgt[(size_t)blk * N + j] : 1.0) * Lm[t + (size_t)j * N] * DZ[(size_t)j * m + r];
                Cxz[e] = 0.5 * sum;
            }
            __syncthreads();
            if (a.emit == 4) {
                // innovation and its covariance for a caller-side significance test: Xout [B][m*m + m] = S (column-major),
                // innovation; nothing else happens
                double *o = a.Xout + (size_t)bidx * (m * m + m);
                for (int e = tid; e < m * m; e += 256) o[e] = Sm[e];
                for (int e = tid; e < m; e += 256) o[m * m + e] = innov[e];
            } else {
                // S^-1 (:285-286): S = 1/2 dZ dZ^T + R is SPD for a valid R -> its Cholesky factor G (m x m, column-major)
                for (int e = tid; e < m * m; e += 256) G[e] = Sm[e];
                const int sfail = general_cholesky(G, m, tid, &ish[45]);
                if (sfail >= 0) {
                    status |= SLK_ST_SINGULAR;
                } else {
                    for (int t = tid; t < N; t += 256) {             // K = covXZ * S^-1 (:288), row t: two triangular solves
                        for (int c = 0; c < m; ++c) {
                            double sum = Cxz[t + (size_t)N * c];
                            for (int p = 0; p < c; ++p) sum -= G[c + m * p] * K[t + (size_t)N * p];
                            K[t + (size_t)N * c] = sum / G[c + m * c];
                        }
                        for (int c = m - 1; c >= 0; --c) {
                            double sum = K[t + (size_t)N * c];
                            for (int p = c + 1; p < m; ++p) sum -= G[p + m * c] * K[t + (size_t)N * p];
                            K[t + (size_t)N * c] = sum / G[c + m * c];
                        }
                    }
                    if (tid == 0) {                                  // mahalanobis2 = |Ls^-1 innovation|^2 (:292)
                        double d2 = 0.0;
                        for (int c = 0; c < m; ++c) {
                            double sum = innov[c];
                            for (int p = 0; p < c; ++p) sum -= G[c + m * p] * wv[p];
                            wv[c] = sum / G[c + m * c];
                            d2 += wv[c] * wv[c];
                        }
                        bool ok = true;
                        if (a.gate > 0) {
                            const double thr[10] = {0, 3.84, 5.99, 7.81, 9.49, 11.07, 12.59, 14.07, 15.51, 16.92};
                            ok = (a.gate <= 9) ? (d2 < thr[a.gate]) : false;   // Usckf.hpp:794-855
                        }
                        ish[40] = ok ? 1 : 0;
                    }
                    __syncthreads();
                    if (!ish[40]) {
                        if (tid == 0) a.outliers[bidx] = 1u;
                        status |= SLK_ST_ALL_REJECTED;
                    } else {
                        for (int t = tid; t < N; t += 256) {         // K * innovation (:299)
                            double sum = 0.0;
                            for (int c = 0; c < m; ++c) sum += K[t + (size_t)N * c] * innov[c];
                            dlt[t] = sum;
                        }
                        // Pk -= K S K^T (:296; K S = covXZ): the lower triangle read, both triangles written from one value
                        for (size_t e = tid; e < (size_t)N * N; e += 256) {
                            const int i = (int)(e % N), j = (int)(e / N);
                            if (i < j) continue;
                            double sum = 0.0;
                            for (int c = 0; c < m; ++c) sum += Cxz[i + (size_t)N * c] * K[j + (size_t)N * c];
                            const double v = gP[e] - sum;
                            gP[e] = v;
                            gP[j + (size_t)i * N] = v;
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
    }
    if (tid == 0 && status) atomicOr(a.status + bidx, status);
}

} // namespace slk
