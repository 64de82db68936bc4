// slk_usckf_general.hpp -- localization::Usckf::predict (reference src/filters/Usckf.hpp:107-244) for states of ANY size:
// the shapes beyond the LDS-resident usckf_kernel (N = 36 + nfk + nfkl > 96; the two feature blocks are dynamic,
// State.hpp:529-593, Usckf.hpp:322-389).  usckf_predict_general_kernel (one wave per filter): the 12-DOF prediction of
// statek_i (predict_phase), Fk = Pxy^T Pk_i^-1 (:154) and the cross blocks (:154-235), streamed one column of P per lane
// -- nothing N-sized is staged.  Emit 1 (predict sigma points) and Y from the caller (SLK_MODEL_EXTERNAL) as in
// usckf_kernel<NT, 256>.  Every update-side call at this N runs on usckf_update_wide_kernel (slk_usckf_wide.hpp).
#pragma once
// (included at the end of slk_usckf.hpp: uses the helpers of slk_kernels.hpp)

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

} // namespace slk
