// slk_ekf_model.hpp -- linearisation of a registered measurement model at the resident mean, for the Msckf EKF update
// (reference src/filters/Msckf.hpp:284-349: the functor h(mu_state, H) of :310, evaluated on the device).
//
// SLK_MM_FEATURE_PROJ, feature j = (landmark Lw, pose index c), pose position p, orientation q, l = R(q)^T (Lw - p):
//   zmean[2j .. 2j+1]           = (l.x / l.z, l.y / l.z)            the arithmetic of measure_item for sigma point 0
//   H[2j .. 2j+1, tp .. tp+2]   = -J R(q)^T                         d/d(position), boxplus p + dp       (State.hpp:186-200)
//   H[2j .. 2j+1, tp+3 .. tp+5] =  J [l]x                           d/d(orientation), boxplus q exp(dtheta) (:286-296)
//   J = [[1/l.z, 0, -l.x/l.z^2], [0, 1/l.z, -l.y/l.z^2]], tp = the pose's tangent offset (pose_of); every other entry of
//   the two rows is an exact +0.0.
// One workgroup per filter.  Phase 1: thread j < m/2 computes the 2 x 6 block of feature j into LDS.  Phase 2: the whole
// m x N column-major matrix is written flat, lane = row within a column, so every wave stores 512 contiguous bytes; the
// zeros are written here (no memset launch).  Plain vector stores only.
// A pose index outside 0 .. k (or NaN) in any feature of a filter: SLK_ST_BAD_INDEX on that filter, its zmean / H are
// filled with NaN and skip[b] is set, which makes the EKF kernels leave the filter untouched (EkfArgs::skip).
#pragma once
#include "slk_kernels.hpp"

namespace slk {

struct LinArgs {
    int B, N, Nq, k, m;
    const double *mean;                 // [B][Nq]
    const double *mp;                   // [B or 1][mp_stride]: (m/2) x { landmark xyz, pose index }
    int mp_stride;
    double *zmean, *H;                  // [B][m], [B][m*N] column-major
    int *status;                        // [B], OR-accumulated
    int *skip;                          // [B] or NULL: 1 = a pose index of this filter is out of range
};

constexpr int LIN_THREADS = 256;        // m <= 512: at most 256 features, one thread each in phase 1

__global__ __launch_bounds__(LIN_THREADS) void msckf_ekf_linearize_kernel(LinArgs a)
{
    __shared__ double blk[LIN_THREADS * 12];      // feature j: row 0 at 12 j, row 1 at 12 j + 6; columns tp .. tp + 5
    __shared__ double zl[LIN_THREADS * 2];
    __shared__ int tpo[LIN_THREADS];
    __shared__ int bad;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = a.N, m = a.m, nf = m >> 1;
    const double *mu = a.mean + (size_t)b * a.Nq;
    const double *mp = a.mp + (size_t)b * a.mp_stride;
    double *zm = a.zmean + (size_t)b * m, *H = a.H + (size_t)b * m * N;
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid < nf) {
        const double c = mp[4 * tid + 3];
        if (!(c >= 0.0 && c <= (double)a.k)) {    // false for NaN
            bad = 1;
        } else {
            Lay L;
            L.kind = SLK_MSCKF; L.k = a.k; L.N = N; L.Nq = a.Nq;
            int tp, sp, sb;
            pose_of(L, (int)c, tp, sp, sb);
            const Quat qc = qconj(ldq(mu + sp + 3));
            double lx, ly, lz;
            qrot(qc, mp[4 * tid] - mu[sp], mp[4 * tid + 1] - mu[sp + 1], mp[4 * tid + 2] - mu[sp + 2], lx, ly, lz);
            zl[2 * tid] = lx / lz;
            zl[2 * tid + 1] = ly / lz;
            const double iz = 1.0 / lz, jx = -lx * iz * iz, jy = -ly * iz * iz;      // J = [[iz, 0, jx], [0, iz, jy]]
            double *h0 = blk + 12 * tid, *h1 = h0 + 6;
            const double ex[3] = {1.0, 0.0, 0.0}, ey[3] = {0.0, 1.0, 0.0}, ez[3] = {0.0, 0.0, 1.0};
#pragma unroll
            for (int i = 0; i < 3; ++i) {         // column i of R(q)^T
                double rx, ry, rz;
                qrot(qc, ex[i], ey[i], ez[i], rx, ry, rz);
                h0[i] = -(iz * rx + jx * rz);
                h1[i] = -(iz * ry + jy * rz);
            }
            // J [l]x, [l]x = [[0, -lz, ly], [lz, 0, -lx], [-ly, lx, 0]]
            h0[3] = -jx * ly;          h0[4] = -iz * lz + jx * lx;   h0[5] = iz * ly;
            h1[3] = iz * lz - jy * ly; h1[4] = jy * lx;              h1[5] = -iz * lx;
            tpo[tid] = tp;
        }
    }
    __syncthreads();
    const bool isbad = bad != 0;
    if (tid == 0) {
        if (a.skip) a.skip[b] = isbad ? 1 : 0;
        if (isbad) atomicOr(a.status + b, (int)SLK_ST_BAD_INDEX);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int r = tid; r < m; r += LIN_THREADS) zm[r] = isbad ? nan : zl[r];
    // The LDS reads below are unconditional on purpose (the store loop stays branch-free, the selects follow): outside the
    // six columns of the row's pose blk is read at offset 0 of the row's block and the value dropped for +0.0; for a bad
    // filter tpo[0] / blk may never have been written, and whatever is read is dropped for NaN.  Every index is in range.
    for (int e = tid; e < m * N; e += LIN_THREADS) {
        const int col = e / m, row = e - col * m, j = row >> 1;
        const int d = col - tpo[isbad ? 0 : j];
        const bool in = (unsigned)d < 6u;
        const double v = blk[12 * j + 6 * (row & 1) + (in ? d : 0)];
        H[e] = isbad ? nan : (in ? v : 0.0);
    }
}

} // namespace slk
