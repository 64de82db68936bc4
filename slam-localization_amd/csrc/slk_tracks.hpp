// slk_tracks.hpp -- Msckf feature-track update: triangulation and null-space marginalisation on the device.
//
// The reference has no such call (its h(mu_state, H) is a host functor); this is the multi-state-constraint measurement
// the sliding window is kept for.  A track is one landmark of UNKNOWN position seen as normalised image points (u, v)
// from several poses of the window (slot = { pose index c, u, v }; c as in SLK_MM_FEATURE_PROJ, c = -1 an empty slot).
// Per track, from the resident mean (include/slk.h spells the steps out, tests/tracks_ref.py follows them in numpy):
//   1. the observed slots; fewer than two: flag 0; a pose named twice: flag -1
//   2. X = (sum (I - d d^T))^-1 sum (I - d d^T) p,  d = R(q) (u, v, 1) normalised, by a 3 x 3 Cholesky
//   3. five Gauss-Newton iterations on e = pi(R^T (X - p)) - (u, v), no early exit
//   4. r = (u, v) - pi(l), H_x = the 2 x 6 block of SLK_MM_FEATURE_PROJ with Lw = X, H_f = J R^T
//   5. three Householder reflections on H_f (the reflector convention of slk_ekf.hpp) applied to [H_x | r], the first
//      three rows dropped, the other 2M - 3 divided by sigma: rows j (2M - 3) .. of the outputs, measurement noise I
//   6. chi2 != NULL: gamma = r^T (H P H^T + I)^-1 r on those rows against chi2[2 n_obs - 3]; not below: flag -2
// The outputs are the (z - zmean, H) pair the EKF kernels (slk_ekf.hpp, slk_ekf_tiles.hpp) take with R = I.
//
// One workgroup per filter, one wave per track (wave w takes tracks w, w + W, ...).  Steps 1 - 4 run with lane = slot:
// the 3 x 3 normal equations are wave reductions (xor butterfly: every lane ends with the same bits and solves them
// itself).  Step 5 runs H_f and r with lane = row in registers (norms and products by wave reductions) and H_x with
// lane = compact column (6 slot + d) through the wave's LDS block, column-major with an odd leading dimension 2M + 1:
// lanes along columns and lanes along rows are both conflict-free.  Columns of empty slots are never touched.
// Step 6 reads P's lower triangle only, four rows of H P per pass, then S column by column; its Cholesky is
// left-looking with lane = row and r as one more row, so the forward substitution comes with it.
// The stores: lane along the rows of the column-major m x N output, zeros included; the padding rows by the whole
// workgroup.  Every entry of r, H and feat is stored exactly once; plain vector stores only.
// A pose index outside -1 .. k (or NaN) anywhere in a filter: SLK_ST_BAD_INDEX, r / H filled with NaN, skip[b] set, as
// msckf_ekf_linearize_kernel does; skip[b] is also set for a filter without a used track.
#pragma once
#include "slk_kernels.hpp"

namespace slk {

struct TrackArgs {
    int B, N, Nq, k, m, J, M, W;        // W waves per workgroup
    const double *mean, *P;             // [B][Nq], [B][N*N] (lower triangle read, and only with chi2)
    const double *tracks;               // [B or 1][t_stride]: J x M x { pose index, u, v }
    int t_stride;
    const double *sigma;                // [B or 1]
    int s_stride;
    const double *chi2;                 // [2M - 2] or NULL
    double *r, *H, *feat;               // [B][m], [B][m*N] column-major, [B][J][4] or NULL
    int *status;                        // [B], OR-accumulated
    int *skip;                          // [B] or NULL
};

constexpr int TRACK_MAX_M = 32;
constexpr int TRACK_MAX_WAVES = 4;
constexpr int TRACK_GATE_ROWS = 4;      // rows of H P formed per pass of the gate

// LDS of one wave in doubles: the block (6M compact columns of H_x + the three reflector vectors), the slot tables
// (pose -> slot, k + 1 ints; slot -> tangent offset, M ints), and for the gate TRACK_GATE_ROWS rows of H P and S with r
__host__ __device__ inline size_t track_wave_doubles(int M, int k, bool gate)
{
    const size_t nr = 2 * (size_t)M - 3;
    size_t n = (6 * (size_t)M + 3) * (2 * (size_t)M + 1) + (k + 2) / 2 + (M + 1) / 2;
    if (gate) n += TRACK_GATE_ROWS * 6 * (size_t)M + nr * (nr + 1);
    return n;
}

__device__ __forceinline__ double track_wsum(double s)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// x = A^-1 b for the symmetric 3 x 3 A given by its lower triangle, by Cholesky; false: a non-positive or NaN pivot
__device__ __forceinline__ bool track_solve3(double a00, double a10, double a11, double a20, double a21, double a22,
                                             double b0, double b1, double b2, double &x0, double &x1, double &x2)
{
    bool ok = a00 > 0.0;
    const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
    const double d1 = a11 - l10 * l10;
    ok = ok && d1 > 0.0;
    const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
    const double d2 = a22 - l20 * l20 - l21 * l21;
    ok = ok && d2 > 0.0;
    const double l22 = sqrt(d2);
    const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = (b2 - l20 * y0 - l21 * y1) / l22;
    x2 = y2 / l22;
    x1 = (y1 - l21 * x2) / l11;
    x0 = (y0 - l10 * x1 - l20 * x2) / l00;
    return ok;
}

// one Householder reflector from column x of the lane = row layout, pivot row kk: beta = -sign(c0) ||x||,
// tau = (beta - c0) / beta, v = x / (c0 - beta) below the pivot, 1 on it, 0 above; tau = 0 for an exactly zero tail
__device__ __forceinline__ void track_reflector(double x, int row, int kk, double &v, double &tau)
{
    const double tail = track_wsum(row > kk ? x * x : 0.0);
    const double c0 = __shfl(x, kk, 64);
    double den = 0.0;
    tau = 0.0;
    if (!(tail <= 2.2250738585072014e-308)) {
        double beta = sqrt(c0 * c0 + tail);
        if (c0 >= 0.0) beta = -beta;
        den = c0 - beta;
        tau = (beta - c0) / beta;
    }
    v = row > kk ? (den != 0.0 ? x / den : 0.0) : (row == kk ? 1.0 : 0.0);
}

__device__ __forceinline__ void track_reflect(double &x, double v, double tau)
{
    const double w = tau * track_wsum(v * x);
    x -= v * w;
}

__global__ __launch_bounds__(64 * TRACK_MAX_WAVES) void msckf_track_linearize_kernel(TrackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double track_lds[];
    __shared__ int s_bad;
    __shared__ int s_used[TRACK_MAX_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = 64 * a.W;
    const int N = a.N, m = a.m, J = a.J, M = a.M, nr = 2 * M - 3, LD = 2 * M + 1, NC = 6 * M;
    const bool gate = a.chi2 != nullptr;
    const double *mu = a.mean + (size_t)b * a.Nq;
    const double *P = a.P + (size_t)b * N * N;
    const double *trk = a.tracks + (size_t)b * a.t_stride;
    const double sg = a.sigma[(size_t)b * a.s_stride];
    double *ro = a.r + (size_t)b * m, *H = a.H + (size_t)b * m * N;
    double *feat = a.feat ? a.feat + (size_t)b * J * 4 : nullptr;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    if (tid == 0) s_bad = 0;
    if (tid < TRACK_MAX_WAVES) s_used[tid] = 0;
    __syncthreads();
    {
        int bad = 0;
        for (int e = tid; e < J * M; e += nthreads) {
            const double c = trk[3 * e];
            if (!(c >= -1.0 && c <= (double)a.k)) bad = 1;        // false for NaN
        }
        if (bad) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {                                                  // uniform over the workgroup
        if (tid == 0) {
            if (a.skip) a.skip[b] = 1;
            atomicOr(a.status + b, (int)SLK_ST_BAD_INDEX);
        }
        for (int e = tid; e < m; e += nthreads) ro[e] = nan;
        for (int e = tid; e < m * N; e += nthreads) H[e] = nan;
        if (feat) for (int e = tid; e < 4 * J; e += nthreads) feat[e] = (e & 3) == 3 ? 0.0 : nan;
        return;
    }

    double *blk = track_lds + (size_t)wave * track_wave_doubles(M, a.k, gate);
    double *vcol = blk + (size_t)NC * LD;                         // v0, v1, v2: LD each
    int *sop = reinterpret_cast<int *>(vcol + 3 * LD);            // pose index -> slot, -1 = not observed
    int *stp = sop + 2 * ((a.k + 2) / 2);                         // slot -> tangent offset
    double *tb = reinterpret_cast<double *>(stp + 2 * ((M + 1) / 2));
    double *S = tb + TRACK_GATE_ROWS * NC;                        // (nr + 1) x nr, column-major: row nr = r
    const int ldS = nr + 1;
    Lay L;
    L.kind = SLK_MSCKF; L.k = a.k; L.N = N; L.Nq = a.Nq;
    int nused = 0;

    for (int j = wave; j < J; j += a.W) {
        const double *tk = trk + (size_t)3 * M * j;
        double c = -1.0, u = 0.0, v = 0.0;
        if (lane < M) { c = tk[3 * lane]; u = tk[3 * lane + 1]; v = tk[3 * lane + 2]; }
        const bool valid = c >= 0.0;
        const int ci = valid ? (int)c : 0;
        const unsigned long long vmask = __ballot(valid);
        const int nobs = __popcll(vmask);
        int tp, sp, sb;
        pose_of(L, ci, tp, sp, sb);
        int flag = 1;
        double X0 = 0.0, X1 = 0.0, X2 = 0.0;
        double f00 = 0.0, f01 = 0.0, f02 = 0.0, f10 = 0.0, f11 = 0.0, f12 = 0.0, r0 = 0.0, r1 = 0.0;
        if (nobs < 2) {
            flag = 0;
        } else {
            bool dup = false;
            for (int t = 0; t < M; ++t) {
                const double ct = __shfl(c, t, 64);
                dup = dup || (valid && t != lane && ct >= 0.0 && (int)ct == ci);
            }
            if (__any(dup)) flag = -1;
        }
        if (flag == 1) {                                          // uniform over the wave from here on
            const double px = mu[sp], py = mu[sp + 1], pz = mu[sp + 2];
            const Quat q = ldq(mu + sp + 3), qc = qconj(q);
            double t00, t10, t20, t01, t11, t21, t02, t12, t22;   // R(q)^T, column i = R^T e_i
            qrot(qc, 1.0, 0.0, 0.0, t00, t10, t20);
            qrot(qc, 0.0, 1.0, 0.0, t01, t11, t21);
            qrot(qc, 0.0, 0.0, 1.0, t02, t12, t22);
            // ---- 2. linear start
            bool ok;
            {
                double dx, dy, dz;
                qrot(q, u, v, 1.0, dx, dy, dz);
                const double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
                dx *= inv; dy *= inv; dz *= inv;
                const double m00 = 1.0 - dx * dx, m10 = -dx * dy, m11 = 1.0 - dy * dy, m20 = -dx * dz, m21 = -dy * dz,
                             m22 = 1.0 - dz * dz;
                const double a00 = track_wsum(valid ? m00 : 0.0), a10 = track_wsum(valid ? m10 : 0.0),
                             a11 = track_wsum(valid ? m11 : 0.0), a20 = track_wsum(valid ? m20 : 0.0),
                             a21 = track_wsum(valid ? m21 : 0.0), a22 = track_wsum(valid ? m22 : 0.0);
                const double b0 = track_wsum(valid ? m00 * px + m10 * py + m20 * pz : 0.0),
                             b1 = track_wsum(valid ? m10 * px + m11 * py + m21 * pz : 0.0),
                             b2 = track_wsum(valid ? m20 * px + m21 * py + m22 * pz : 0.0);
                ok = track_solve3(a00, a10, a11, a20, a21, a22, b0, b1, b2, X0, X1, X2);
            }
            // ---- 3. five Gauss-Newton iterations, then 4. the residual and the Jacobians at the final X
            double lx = 0.0, ly = 0.0, lz = 1.0, iz = 1.0, jx = 0.0, jy = 0.0;
            for (int it = 0; it <= 5; ++it) {
                qrot(qc, X0 - px, X1 - py, X2 - pz, lx, ly, lz);
                iz = 1.0 / lz; jx = -lx * iz * iz; jy = -ly * iz * iz;           // J = [[iz, 0, jx], [0, iz, jy]]
                f00 = iz * t00 + jx * t20; f01 = iz * t01 + jx * t21; f02 = iz * t02 + jx * t22;
                f10 = iz * t10 + jy * t20; f11 = iz * t11 + jy * t21; f12 = iz * t12 + jy * t22;
                r0 = u - lx / lz; r1 = v - ly / lz;
                if (it == 5) break;
                const double g00 = track_wsum(valid ? f00 * f00 + f10 * f10 : 0.0), g10 = track_wsum(valid ? f01 * f00 + f11 * f10 : 0.0),
                             g11 = track_wsum(valid ? f01 * f01 + f11 * f11 : 0.0), g20 = track_wsum(valid ? f02 * f00 + f12 * f10 : 0.0),
                             g21 = track_wsum(valid ? f02 * f01 + f12 * f11 : 0.0), g22 = track_wsum(valid ? f02 * f02 + f12 * f12 : 0.0);
                const double h0 = track_wsum(valid ? -(f00 * r0 + f10 * r1) : 0.0),  // F^T e, e = -r
                             h1 = track_wsum(valid ? -(f01 * r0 + f11 * r1) : 0.0),
                             h2 = track_wsum(valid ? -(f02 * r0 + f12 * r1) : 0.0);
                double d0, d1, d2;
                ok = track_solve3(g00, g10, g11, g20, g21, g22, h0, h1, h2, d0, d1, d2) && ok;
                X0 -= d0; X1 -= d1; X2 -= d2;
            }
            const double fin = (X0 - X0) + (X1 - X1) + (X2 - X2);              // 0 for a finite X, NaN otherwise
            if (!ok || !(fin == 0.0) || __any(valid && !(lz > 0.0))) flag = -1;
            if (flag == 1) {
                // ---- 5. marginalisation.  The slots publish their 2 x 6 blocks and tables, then lane = row
                if (!valid) { f00 = f01 = f02 = f10 = f11 = f12 = r0 = r1 = 0.0; }
                for (int e = lane; e <= a.k; e += 64) sop[e] = -1;
                wave_sync();
                if (valid) {
                    double *c0 = blk + (size_t)(6 * lane) * LD + 2 * lane;
                    c0[0] = -f00;                   c0[1] = -f10;
                    c0[LD] = -f01;                  c0[LD + 1] = -f11;
                    c0[2 * LD] = -f02;              c0[2 * LD + 1] = -f12;
                    // J [l]x, [l]x = [[0, -lz, ly], [lz, 0, -lx], [-ly, lx, 0]]
                    c0[3 * LD] = -jx * ly;          c0[3 * LD + 1] = iz * lz - jy * ly;
                    c0[4 * LD] = -iz * lz + jx * lx; c0[4 * LD + 1] = jy * lx;
                    c0[5 * LD] = iz * ly;           c0[5 * LD + 1] = -iz * lx;
                    sop[ci] = lane;
                    stp[lane] = tp;
                }
                const int row = lane, src = (lane >> 1) & 31;
                const bool odd = lane & 1;
                double hf0, hf1, hf2, rr;
                {
                    const double e0 = __shfl(f00, src, 64), o0 = __shfl(f10, src, 64), e1 = __shfl(f01, src, 64), o1 = __shfl(f11, src, 64);
                    const double e2 = __shfl(f02, src, 64), o2 = __shfl(f12, src, 64), er = __shfl(r0, src, 64), orr = __shfl(r1, src, 64);
                    const bool in = row < 2 * M;
                    hf0 = in ? (odd ? o0 : e0) : 0.0;
                    hf1 = in ? (odd ? o1 : e1) : 0.0;
                    hf2 = in ? (odd ? o2 : e2) : 0.0;
                    rr = in ? (odd ? orr : er) : 0.0;
                }
                double v0, v1, v2, tau0, tau1, tau2;
                track_reflector(hf0, row, 0, v0, tau0);
                track_reflect(hf1, v0, tau0); track_reflect(hf2, v0, tau0); track_reflect(rr, v0, tau0);
                track_reflector(hf1, row, 1, v1, tau1);
                track_reflect(hf2, v1, tau1); track_reflect(rr, v1, tau1);
                track_reflector(hf2, row, 2, v2, tau2);
                track_reflect(rr, v2, tau2);
                rr = rr / sg;
                if (row < 2 * M) { vcol[row] = v0; vcol[LD + row] = v1; vcol[2 * LD + row] = v2; }
                wave_sync();
                for (int cc = lane; cc < NC; cc += 64) {
                    const int s = cc / 6;
                    if (!((vmask >> s) & 1ull)) continue;
                    double *col = blk + (size_t)cc * LD;
                    const double ca = col[2 * s], cb = col[2 * s + 1];
                    const double w0 = tau0 * (vcol[2 * s] * ca + vcol[2 * s + 1] * cb);
                    double dot = 0.0;
                    for (int i = 0; i < 2 * M; ++i) {
                        const double x = (i == 2 * s ? ca : (i == 2 * s + 1 ? cb : 0.0)) - vcol[i] * w0;
                        col[i] = x;
                        dot += vcol[LD + i] * x;
                    }
                    const double w1 = tau1 * dot;
                    dot = 0.0;
                    for (int i = 1; i < 2 * M; ++i) {
                        const double x = col[i] - vcol[LD + i] * w1;
                        col[i] = x;
                        dot += vcol[2 * LD + i] * x;
                    }
                    const double w2 = tau2 * dot;
                    for (int i = 3; i < 2 * M; ++i) col[i] = (col[i] - vcol[2 * LD + i] * w2) / sg;
                }
                wave_sync();
                // ---- 6. the gate
                if (gate) {
                    for (int i0 = 0; i0 < nr; i0 += TRACK_GATE_ROWS) {
                        int rq[TRACK_GATE_ROWS];
#pragma unroll
                        for (int q4 = 0; q4 < TRACK_GATE_ROWS; ++q4) rq[q4] = 3 + (i0 + q4 < nr ? i0 + q4 : nr - 1);
                        for (int bc = lane; bc < NC; bc += 64) {                 // rows i0 .. of H P, lane = column
                            const int s = bc / 6;
                            if (!((vmask >> s) & 1ull)) continue;
                            const int tcol = stp[s] + (bc - 6 * s);
                            double acc[TRACK_GATE_ROWS] = {0.0, 0.0, 0.0, 0.0};
                            for (int sa = 0; sa < M; ++sa) {
                                if (!((vmask >> sa) & 1ull)) continue;
                                const int ta0 = stp[sa];
                                for (int d = 0; d < 6; ++d) {
                                    const int ta = ta0 + d, hi = ta > tcol ? ta : tcol, lo = ta > tcol ? tcol : ta;
                                    const double p = P[(size_t)lo * N + hi];
                                    const double *hc = blk + (size_t)(6 * sa + d) * LD;
#pragma unroll
                                    for (int q4 = 0; q4 < TRACK_GATE_ROWS; ++q4) acc[q4] += hc[rq[q4]] * p;
                                }
                            }
#pragma unroll
                            for (int q4 = 0; q4 < TRACK_GATE_ROWS; ++q4) tb[q4 * NC + bc] = acc[q4];
                        }
                        wave_sync();
                        if (lane < nr) {                                         // S(i0 .., lane) = (H P) H^T + I
                            double acc[TRACK_GATE_ROWS] = {0.0, 0.0, 0.0, 0.0};
                            for (int sa = 0; sa < M; ++sa) {
                                if (!((vmask >> sa) & 1ull)) continue;
                                for (int d = 0; d < 6; ++d) {
                                    const int bc = 6 * sa + d;
                                    const double hb = blk[(size_t)bc * LD + 3 + lane];
#pragma unroll
                                    for (int q4 = 0; q4 < TRACK_GATE_ROWS; ++q4) acc[q4] += tb[q4 * NC + bc] * hb;
                                }
                            }
#pragma unroll
                            for (int q4 = 0; q4 < TRACK_GATE_ROWS; ++q4) {
                                const int i = i0 + q4;
                                if (i < nr && lane <= i) S[(size_t)lane * ldS + i] = acc[q4] + (lane == i ? 1.0 : 0.0);
                            }
                        }
                        wave_sync();
                    }
                    if (row >= 3 && row < 2 * M) S[(size_t)(row - 3) * ldS + nr] = rr;
                    wave_sync();
                    double gam = 0.0;
                    bool gok = true;
                    for (int jc = 0; jc < nr; ++jc) {                            // left-looking, lane = row, row nr = r
                        double s = 0.0;
                        const bool mine = lane >= jc && lane <= nr;
                        if (mine) {
                            s = S[(size_t)jc * ldS + lane];
                            for (int p = 0; p < jc; ++p) s -= S[(size_t)p * ldS + lane] * S[(size_t)p * ldS + jc];
                        }
                        const double d = __shfl(s, jc, 64);
                        gok = gok && d > 0.0;
                        const double sd = sqrt(d), val = lane == jc ? sd : s / sd;
                        if (mine) S[(size_t)jc * ldS + lane] = val;
                        if (lane == nr) gam += val * val;
                        wave_sync();
                    }
                    gam = __shfl(gam, nr, 64);
                    if (!(gok && gam < a.chi2[2 * nobs - 3])) flag = -2;
                }
                // ---- the rows of this track, lane along the rows of the column-major output
                if (flag == 1) {
                    const int R0 = j * nr;
                    if (row >= 3 && row < 2 * M) ro[R0 + row - 3] = rr;
                    for (int e = lane; e < nr * N; e += 64) {
                        const int col = e / nr, i = e - col * nr;
                        const int pc = col < 6 ? 0 : (col < 12 ? -1 : 1 + (col - 12) / 6);
                        const int d = col < 6 ? col : (col - 12) % 6;
                        const int s = pc < 0 ? -1 : sop[pc];
                        H[(size_t)col * m + R0 + i] = s < 0 ? 0.0 : blk[(size_t)(6 * s + d) * LD + 3 + i];
                    }
                    nused++;
                }
                wave_sync();                                      // the next track reuses the block
            }
        }
        if (flag != 1) {
            const int R0 = j * nr;
            for (int e = lane; e < nr; e += 64) ro[R0 + e] = 0.0;
            for (int e = lane; e < nr * N; e += 64) {
                const int col = e / nr, i = e - col * nr;
                H[(size_t)col * m + R0 + i] = 0.0;
            }
        }
        if (feat && lane == 0) {
            const bool point = flag == 1 || flag == -2;
            feat[4 * j] = flag == 0 ? 0.0 : (point ? X0 : nan);
            feat[4 * j + 1] = flag == 0 ? 0.0 : (point ? X1 : nan);
            feat[4 * j + 2] = flag == 0 ? 0.0 : (point ? X2 : nan);
            feat[4 * j + 3] = (double)flag;
        }
    }
    // the padding rows, and the skip flag of a filter without a used track
    const int pad = m - J * nr;
    for (int e = tid; e < pad; e += nthreads) ro[J * nr + e] = 0.0;
    for (int e = tid; e < pad * N; e += nthreads) {
        const int col = e / pad, i = e - col * pad;
        H[(size_t)col * m + J * nr + i] = 0.0;
    }
    if (lane == 0) s_used[wave] = nused;
    __syncthreads();
    if (tid == 0 && a.skip) {
        int n = 0;
        for (int w = 0; w < a.W; ++w) n += s_used[w];
        a.skip[b] = n == 0 ? 1 : 0;
    }
}

// R = I_m of the EKF update that follows (column-major, m * m doubles)
__global__ __launch_bounds__(256) void track_identity_kernel(double *I, int m)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < m * m) I[e] = (e / m == e % m) ? 1.0 : 0.0;
}

} // namespace slk
