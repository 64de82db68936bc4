// slk_ensemble.hpp -- what crosses the filters of a batch: the moments of the batch or of G groups of it
// (slk_ensemble_moments: a centre, the between-filter spread, the weighted mean of the filters' covariances) and a gather
// of whole filters (slk_gather_states: resampling, pruning, fan-out).  The reference has neither; both reuse its manifold
// operators (State.hpp:186-200 through the layout helpers of slk_kernels.hpp), in the LEAF forms, as slk_consistency.hpp.
// Group g is the filters [g Bg, (g + 1) Bg), Bg = B / G.  Every sum over filters is taken in a fixed order: a thread walks
// its filters in index order, the threads / waves of a workgroup are added in index order, the chunks of a group are
// added in index order by ens_reduce_kernel -- no atomics, and the chunking (ens_plan) depends on (B, G, N, n) only, so
// two calls on the same state give the same bits on any device.
//   weights:   wn [B] = w_b / sum_group w, ess [G] = (sum w)^2 / sum w^2; a group with a negative, NaN or infinite weight
//              or a sum that is not > 0 gets wn = NaN, which makes every output of that group NaN with no further test.
//   centre:    mixture mode, one 512-thread workgroup per group runs the whole pinned iteration ref <- ref [+] dbar,
//              dbar = sum wn_b (mu_b [-] ref), in one launch (no host synchronisation between passes).
//   deviations D [B][n]: truth_b [-] mu_b (error mode) or mu_b [-] centre (mixture mode) on the range; the bias (error
//              mode) is their weighted mean (ens_bias_kernel).
//   spread:    D' diag(wn) D'^T, D' = D - bias, a tall-skinny SYRK over the filter index on fp64 MFMA (16 x 16 x 4, the
//              operand / result maps of wide_mfma_k and chol_blocked_mem: A[lane & 15][k = lane >> 4], C col = lane & 15,
//              row = (lane >> 4) + 4 reg).  Lower tiles only; one workgroup = one tile x ENS_SPREAD_K filters, 64 per wave.
//   mean cov:  the streaming pass.  A thread owns one entry of the packed lower triangle of the range's sub-block and
//              walks the filters of its chunk (consecutive threads = consecutive rows of a column of the column-major P).
//              Reads the LOWER triangle of P only.
// Partials are packed lower triangles [G][chunks][E], E = n (n + 1) / 2; a pass with one chunk per group writes its
// output directly.  Outputs are full n x n column-major, both triangles written from one value.
//   gather:    filter b <- old filter src[b]: mean, P (whole, or as its lower triangle when the covariance is lower-only),
//              status bits and outlier count, out of place into the handle's second buffers.
// The kernels are compiled in a translation unit of their own (slk_ensemble.hip, SLK_ENSEMBLE_UNIT); slk_api.hip sees
// the plan and the declarations only, so the device code of its kernels is what it was without them.
#pragma once
// (included after slk_kernels.hpp)

namespace slk {

constexpr int ENS_COV_WGS = 2048;      // workgroups the mean-covariance pass aims for
constexpr int ENS_COV_MIN = 8;         // least filters per chunk of it
constexpr int ENS_COV_UNROLL = 8;      // independent loads in flight per thread
constexpr int ENS_SPREAD_K = 256;      // filters per workgroup of the spread pass (64 per wave, 16 k-steps)
constexpr int ENS_CENTRE_THREADS = 512, ENS_CENTRE_TX = 16, ENS_CENTRE_TY = ENS_CENTRE_THREADS / ENS_CENTRE_TX;
constexpr int ENS_CENTRE_UNROLL = 4;   // filters whose loads a thread of the centre kernel keeps in flight
constexpr int ENS_SUM_UNROLL = 8;      // the same for the bias and the final reduce
constexpr int GATHER_UNROLL = 8, GATHER_CHUNK = 256 * GATHER_UNROLL;

// workspace of slk_ensemble_moments (doubles) and the chunking of its two reductions: a function of (B, G, N, Nq, n)
// and the mode only
struct EnsPlan {
    int Bg, E, ldc;                    // filters per group, packed entries of the range, row length of the centre
    int cov_chunks, cov_fc;            // mean covariance: chunks per group, filters per chunk
    int spr_chunks;                    // spread: chunks per group
    size_t w_raw, wn, ess, centre, D, pcov, pspr, total;
};
__host__ __device__ inline EnsPlan ens_plan(int B, int G, int Nq, int n, bool mixture)
{
    EnsPlan p;
    p.Bg = B / G;
    p.E = n * (n + 1) / 2;
    p.ldc = mixture ? Nq : n;
    const long long eb = (p.E + 255) / 256;
    long long c = (ENS_COV_WGS + eb * G - 1) / (eb * G);
    const long long cmax = (p.Bg + ENS_COV_MIN - 1) / ENS_COV_MIN;
    if (c > cmax) c = cmax;
    if (c < 1) c = 1;
    p.cov_fc = (int)((p.Bg + c - 1) / c);
    p.cov_chunks = (p.Bg + p.cov_fc - 1) / p.cov_fc;
    p.spr_chunks = (p.Bg + ENS_SPREAD_K - 1) / ENS_SPREAD_K;
    size_t o = 0;
    p.w_raw = o;  o += (size_t)B;                                 // the weights of a host call
    p.wn = o;     o += (size_t)B;
    p.ess = o;    o += (size_t)G;
    p.centre = o; o += (size_t)G * p.ldc;
    p.D = o;      o += (size_t)B * n;
    p.pcov = o;   o += p.cov_chunks > 1 ? (size_t)G * p.cov_chunks * p.E : 0;
    p.pspr = o;   o += p.spr_chunks > 1 ? (size_t)G * p.spr_chunks * p.E : 0;
    p.total = (o + 7) & ~(size_t)7;
    return p;
}
// dynamic LDS of ens_centre_kernel (bytes): ref [Nq], dbar [N], the partial sums of one tile of tangent indices
__host__ __device__ inline size_t ens_centre_lds(int N, int Nq)
{
    return ((size_t)round_up(Nq, 2) + round_up(N, 2) + ENS_CENTRE_THREADS) * sizeof(double);
}
// elements the gather moves per filter: the whole matrix, or the lower triangle with the columns taken in pairs
// (c, N - 1 - c) of N + 1 elements (two contiguous runs each) and, for odd N, the middle column on its own
__host__ __device__ inline long long gather_elems(int N, int lower)
{
    return lower ? (long long)(N / 2) * (N + 1) + ((N & 1) ? (N + 1) / 2 : 0) : (long long)N * N;
}

__global__ void ens_weights_kernel(const double *w, int Bg, double *wn, double *ess);
__global__ void ens_centre_kernel(Lay L, const double *mean, const double *wn, int Bg, double *centre);
__global__ void ens_dev_kernel(Lay L, const double *mean, const double *truth, const double *centre, int B, int Bg, int t0,
                               int n, double *D);
__global__ void ens_bias_kernel(const double *D, const double *wn, int Bg, int n, double *centre);
__global__ void ens_spread_kernel(const double *D, const double *wn, const double *sub, int Bg, int n, int chunks,
                                  double *partial, double *out);
__global__ void ens_meancov_kernel(const double *P, const double *wn, int N, int t0, int n, int Bg, int fc, int chunks,
                                   double *partial, double *out);
__global__ void ens_reduce_kernel(const double *partial0, int chunks0, double *out0, const double *partial1, int chunks1,
                                  double *out1, int n);
__global__ void gather_states_kernel(const double *mean, const double *P, const int *status, const unsigned *outliers,
                                     const int *src, double *nmean, double *nP, int *nstatus, unsigned *noutliers, int B,
                                     int N, int Nq, int lower);

#ifdef SLK_ENSEMBLE_UNIT
// component `comp` of the 3-vector a [-] b = log(b^-1 a) of SO(3) block `blk`, the libm routes inlined (the reason:
// slk_consistency.hpp)
__device__ __forceinline__ double ens_so3_minus(const Lay &L, const double *a, const double *b, int blk, int comp)
{
    double d0, d1, d2;
    so3_log<true>(qmul(qconj(ldq(b + so3_soff(L, blk))), ldq(a + so3_soff(L, blk))), d0, d1, d2);
    return comp == 0 ? d0 : (comp == 1 ? d1 : d2);
}
// (a [-] b)(t), any tangent index
__device__ __forceinline__ double ens_minus(const Lay &L, const double *a, const double *b, int t)
{
    int blk = 0, comp = 0;
    const int s = t2s(L, t, blk, comp);
    return s >= 0 ? a[s] - b[s] : ens_so3_minus(L, a, b, blk, comp);
}

// first element of column j of the packed lower triangle (pk(n, j, j)), and entry e -> (i, j), i >= j
__device__ __forceinline__ int ens_colstart(int n, int j) { return (j * (2 * n - j + 1)) >> 1; }
__device__ __forceinline__ void ens_unpack(int n, int e, int &i, int &j)
{
    const double t = 2.0 * n + 1.0;
    int c = (int)((t - sqrt(t * t - 8.0 * e)) * 0.5);
    c = c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
    while (c > 0 && ens_colstart(n, c) > e) --c;
    while (c + 1 < n && ens_colstart(n, c + 1) <= e) ++c;
    j = c;
    i = c + (e - ens_colstart(n, c));
}

// sum of one value per thread of a 256-thread workgroup, in thread order by halves: the same order every time
__device__ __forceinline__ double ens_block_sum(double x, double *red, int tid)
{
    red[tid] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();                                           // (red is reused)
    return r;
}

// grid G, 256 threads.  w null = uniform.
__global__ __launch_bounds__(256) void ens_weights_kernel(const double *w, int Bg, double *wn, double *ess)
{
    __shared__ double red[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)g * Bg;
    double s = 0.0, s2 = 0.0, bad = 0.0;
    for (int b = tid; b < Bg; b += 256) {
        const double x = w ? w[base + b] : 1.0;
        if (!(x >= 0.0) || x > 0x1.fffffffffffffp1023) bad = 1.0;   // negative, NaN, infinite
        s += x;
        s2 = fma(x, x, s2);
    }
    const double sum = ens_block_sum(s, red, tid);
    const double sum2 = ens_block_sum(s2, red, tid);
    const double nbad = ens_block_sum(bad, red, tid);
    const bool ok = nbad == 0.0 && sum > 0.0 && sum <= 0x1.fffffffffffffp1023;
    for (int b = tid; b < Bg; b += 256) wn[base + b] = ok ? (w ? w[base + b] : 1.0) / sum : __builtin_nan("");
    if (tid == 0) ess[g] = ok ? sum * sum / sum2 : __builtin_nan("");
}

// Mixture mode: centre [G][Nq] = the weighted manifold mean of the group's means.  grid G, ENS_CENTRE_THREADS threads,
// dynamic LDS ens_centre_lds.  Thread (tx, ty) takes tangent index 16 tile + tx and the filters ty, ty + 32, ...
__global__ __launch_bounds__(ENS_CENTRE_THREADS) void ens_centre_kernel(Lay L, const double *mean, const double *wn, int Bg,
                                                                        double *centre)
{
    extern __shared__ __attribute__((aligned(16))) double ens_smem[];
    const int g = blockIdx.x, tid = threadIdx.x, N = L.N, Nq = L.Nq;
    const int tx = tid % ENS_CENTRE_TX, ty = tid / ENS_CENTRE_TX;
    double *ref = ens_smem, *dbar = ref + round_up(Nq, 2), *part = dbar + round_up(N, 2);
    const double *mu = mean + (size_t)g * Bg * Nq, *w = wn + (size_t)g * Bg;
    double *out = centre + (size_t)g * Nq;
    if (w[0] != w[0]) {                                        // a refused group: every weight is NaN
        for (int s = tid; s < Nq; s += ENS_CENTRE_THREADS) out[s] = __builtin_nan("");
        return;
    }
    for (int s = tid; s < Nq; s += ENS_CENTRE_THREADS) ref[s] = mu[s];
    __syncthreads();
    for (int pass = 0; pass < 100; ++pass) {
        for (int t0 = 0; t0 < N; t0 += ENS_CENTRE_TX) {
            const int t = t0 + tx;
            double acc = 0.0;
            // the pass is bound by the latency of the loads of mu, not by arithmetic: ENS_CENTRE_UNROLL filters' loads are
            // issued before the first is used; the sum runs in filter order either way
            if (t < N) {
                constexpr int TY = ENS_CENTRE_TY, U = ENS_CENTRE_UNROLL;
                int blk = 0, comp = 0;
                const int s = t2s(L, t, blk, comp);
                int b = ty;
                if (s >= 0) {
                    const double r = ref[s];
                    for (; b + (U - 1) * TY < Bg; b += U * TY) {
                        double v[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) v[u] = mu[(size_t)(b + u * TY) * Nq + s];
#pragma unroll
                        for (int u = 0; u < U; ++u) acc = fma(w[b + u * TY], v[u] - r, acc);
                    }
                    for (; b < Bg; b += TY) acc = fma(w[b], mu[(size_t)b * Nq + s] - r, acc);
                } else {
                    const int so = so3_soff(L, blk);
                    const Quat rc = qconj(ldq(ref + so));
                    auto term = [&](const Quat &q) {
                        double d0, d1, d2;
                        so3_log<true>(qmul(rc, q), d0, d1, d2);
                        return comp == 0 ? d0 : (comp == 1 ? d1 : d2);
                    };
                    for (; b + (U - 1) * TY < Bg; b += U * TY) {
                        Quat q[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) q[u] = ldq(mu + (size_t)(b + u * TY) * Nq + so);
#pragma unroll
                        for (int u = 0; u < U; ++u) acc = fma(w[b + u * TY], term(q[u]), acc);
                    }
                    for (; b < Bg; b += TY) acc = fma(w[b], term(ldq(mu + (size_t)b * Nq + so)), acc);
                }
            }
            part[tid] = acc;
            __syncthreads();
            if (ty == 0 && t < N) {
                double s = 0.0;
                for (int y = 0; y < ENS_CENTRE_TY; ++y) s += part[y * ENS_CENTRE_TX + tx];
                dbar[t] = s;
            }
            __syncthreads();
        }
        double n2 = 0.0;                                       // (every thread the same sum in the same order)
        for (int t = 0; t < N; ++t) n2 = fma(dbar[t], dbar[t], n2);
        for (int t = tid; t < N; t += ENS_CENTRE_THREADS) {   // ref <- ref [+] dbar
            int blk = 0, comp = 0;
            const int s = t2s(L, t, blk, comp);
            if (s >= 0) {
                ref[s] += dbar[t];
            } else if (comp == 0) {
                const int so = so3_soff(L, blk);
                stq(ref + so, qmul(ldq(ref + so), so3_exp<true>(dbar[t], dbar[t + 1], dbar[t + 2])));
            }
        }
        __syncthreads();
        if (sqrt(n2) <= 1e-12) break;
    }
    for (int s = tid; s < Nq; s += ENS_CENTRE_THREADS) out[s] = ref[s];
}

// D [B][n]: (truth_b [-] mu_b)(t0 + i) when truth is given, else (mu_b [-] centre_g)(t0 + i).  grid ceil(B n / 256)
__global__ __launch_bounds__(256) void ens_dev_kernel(Lay L, const double *mean, const double *truth, const double *centre,
                                                      int B, int Bg, int t0, int n, double *D)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * n) return;
    const size_t b = e / n;
    const int i = (int)(e - b * n);
    const double *mu = mean + b * L.Nq;
    D[e] = truth ? ens_minus(L, truth + b * L.Nq, mu, t0 + i) : ens_minus(L, mu, centre + (b / Bg) * L.Nq, t0 + i);
}

// centre [G][n] = sum wn_b D_b (the bias of error mode).  grid ceil(n / 16) G, 256 threads = 16 indices x 16 slices
__global__ __launch_bounds__(256) void ens_bias_kernel(const double *D, const double *wn, int Bg, int n, double *centre)
{
    __shared__ double part[256];
    const int nb = (n + 15) / 16, g = blockIdx.x / nb, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i = (blockIdx.x - g * nb) * 16 + tx;
    const double *Dg = D + (size_t)g * Bg * n, *w = wn + (size_t)g * Bg;
    double acc = 0.0;
    if (i < n) {
        constexpr int U = ENS_SUM_UNROLL;
        int b = ty;
        for (; b + (U - 1) * 16 < Bg; b += U * 16) {            // (loads first: the sum is bound by their latency)
            double v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = Dg[(size_t)(b + u * 16) * n + i];
#pragma unroll
            for (int u = 0; u < U; ++u) acc = fma(w[b + u * 16], v[u], acc);
        }
        for (; b < Bg; b += 16) acc = fma(w[b], Dg[(size_t)b * n + i], acc);
    }
    part[tid] = acc;
    __syncthreads();
    if (ty == 0 && i < n) {
        double s = 0.0;
        for (int y = 0; y < 16; ++y) s += part[y * 16 + tx];
        centre[(size_t)g * n + i] = s;
    }
}

// one value of the lower triangle into a full column-major n x n matrix, both triangles
__device__ __forceinline__ void ens_store_sym(double *M, int n, int i, int j, double v)
{
    M[i + (size_t)j * n] = v;
    M[j + (size_t)i * n] = v;
}

// spread: sum over the chunk's filters of wn_b (D_b - sub)(D_b - sub)^T, lower tiles.  grid (tiles G, chunks), 256 threads;
// tiles = T (T + 1) / 2, T = ceil(n / 16).  sub [G][n] (the bias) or null.  chunks == 1: straight into out [G][n n].
__global__ __launch_bounds__(256) void ens_spread_kernel(const double *D, const double *wn, const double *sub, int Bg, int n,
                                                         int chunks, double *partial, double *out)
{
    __shared__ double tile[4 * 256];
    const int T = (n + 15) / 16, tiles = T * (T + 1) / 2;
    const int g = blockIdx.x / tiles, chunk = blockIdx.y, tid = threadIdx.x;
    int I = 0, rem = blockIdx.x - g * tiles;                   // tile (I, J), J <= I, row by row
    while (rem > I) { rem -= I + 1; ++I; }
    const int J = rem;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
    const double *Dg = D + (size_t)g * Bg * n, *w = wn + (size_t)g * Bg;
    const int i = 16 * I + c, j = 16 * J + c;
    const double si = (sub && i < n) ? sub[(size_t)g * n + i] : 0.0, sj = (sub && j < n) ? sub[(size_t)g * n + j] : 0.0;
    const int k0 = chunk * ENS_SPREAD_K + wave * 64;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kk = 0; kk < 64; kk += 16) {                      // (the k loop of wide_mfma_k: loads of four k-steps first)
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = k0 + kk + 4 * u + q;
            const bool in = b < Bg;
            av[u] = (in && i < n) ? w[b] * (Dg[(size_t)b * n + i] - si) : 0.0;
            bv[u] = (in && j < n) ? Dg[(size_t)b * n + j] - sj : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[wave * 256 + (q + 4 * r) * 16 + c] = acc[r];
    __syncthreads();
    const double v = ((tile[tid] + tile[256 + tid]) + tile[512 + tid]) + tile[768 + tid];
    const int ri = 16 * I + (tid >> 4), cj = 16 * J + (tid & 15);
    if (ri < n && cj <= ri) {
        if (chunks == 1) ens_store_sym(out + (size_t)g * n * n, n, ri, cj, v);
        else partial[((size_t)g * chunks + chunk) * (n * (n + 1) / 2) + ens_colstart(n, cj) + (ri - cj)] = v;
    }
}

// mean covariance: sum over the chunk's filters of wn_b P_b(t0 + i, t0 + j), i >= j.  grid (ceil(E / 256) G, chunks),
// 256 threads, one packed entry per thread.  chunks == 1: straight into out [G][n n].
__global__ __launch_bounds__(256) void ens_meancov_kernel(const double *__restrict__ P, const double *__restrict__ wn, int N,
                                                          int t0, int n, int Bg, int fc, int chunks,
                                                          double *__restrict__ partial, double *__restrict__ out)
{
    const int E = n * (n + 1) / 2, eb = (E + 255) / 256;
    const int g = blockIdx.x / eb, chunk = blockIdx.y;
    const int e = (blockIdx.x - g * eb) * 256 + threadIdx.x;
    if (e >= E) return;
    int i, j;
    ens_unpack(n, e, i, j);
    const int b0 = chunk * fc, b1 = min(b0 + fc, Bg);
    const size_t NN = (size_t)N * N;
    const double *p = P + ((size_t)g * Bg + b0) * NN + (size_t)(t0 + i) + (size_t)(t0 + j) * N;
    const double *w = wn + (size_t)g * Bg;
    double acc = 0.0;
    int b = b0;
    for (; b + ENS_COV_UNROLL <= b1; b += ENS_COV_UNROLL) {
        double v[ENS_COV_UNROLL];
#pragma unroll
        for (int u = 0; u < ENS_COV_UNROLL; ++u) v[u] = p[(size_t)u * NN];
#pragma unroll
        for (int u = 0; u < ENS_COV_UNROLL; ++u) acc = fma(w[b + u], v[u], acc);
        p += (size_t)ENS_COV_UNROLL * NN;
    }
    for (; b < b1; ++b) { acc = fma(w[b], *p, acc); p += NN; }
    if (chunks == 1) ens_store_sym(out + (size_t)g * n * n, n, i, j, acc);
    else partial[((size_t)g * chunks + chunk) * E + e] = acc;
}

// out [G][n n] = the chunks of partial [G][chunks][E] added in index order, for up to two reductions at once (the spread
// and the mean covariance of one call): grid (ceil(E / 256) G, 1 or 2), 256 threads
__global__ __launch_bounds__(256) void ens_reduce_kernel(const double *partial0, int chunks0, double *out0,
                                                         const double *partial1, int chunks1, double *out1, int n)
{
    const int E = n * (n + 1) / 2, eb = (E + 255) / 256, g = blockIdx.x / eb;
    const int e = (blockIdx.x - g * eb) * 256 + threadIdx.x;
    if (e >= E) return;
    const double *partial = blockIdx.y ? partial1 : partial0;
    const int chunks = blockIdx.y ? chunks1 : chunks0;
    double *out = blockIdx.y ? out1 : out0;
    const double *p = partial + (size_t)g * chunks * E + e;
    double s = 0.0;
    int c = 0;
    for (; c + ENS_SUM_UNROLL <= chunks; c += ENS_SUM_UNROLL) {   // (loads first: the sum is bound by their latency)
        double v[ENS_SUM_UNROLL];
#pragma unroll
        for (int u = 0; u < ENS_SUM_UNROLL; ++u) v[u] = p[(size_t)(c + u) * E];
#pragma unroll
        for (int u = 0; u < ENS_SUM_UNROLL; ++u) s += v[u];
    }
    for (; c < chunks; ++c) s += p[(size_t)c * E];
    int i, j;
    ens_unpack(n, e, i, j);
    ens_store_sym(out + (size_t)g * n * n, n, i, j, s);
}

// filter b <- old filter src[b].  grid (B, chunks of GATHER_CHUNK elements of gather_elems), 256 threads; the chunk-0
// workgroup of a filter moves its mean, status word and outlier count.  An index outside 0 .. B - 1 (device-resident
// indices only: the host checks its own) keeps the filter's own state and sets SLK_ST_BAD_INDEX.
__global__ __launch_bounds__(256) void gather_states_kernel(const double *__restrict__ mean, const double *__restrict__ P,
                                                            const int *__restrict__ status,
                                                            const unsigned *__restrict__ outliers,
                                                            const int *__restrict__ src, double *__restrict__ nmean,
                                                            double *__restrict__ nP, int *__restrict__ nstatus,
                                                            unsigned *__restrict__ noutliers, int B, int N, int Nq, int lower)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    int s = src[b];
    const bool bad = s < 0 || s >= B;
    if (bad) s = b;
    if (blockIdx.y == 0) {
        const double *m = mean + (size_t)s * Nq;
        double *mo = nmean + (size_t)b * Nq;
        for (int e = tid; e < Nq; e += 256) mo[e] = m[e];
        if (tid == 0) {
            nstatus[b] = status[s] | (bad ? SLK_ST_BAD_INDEX : 0);
            noutliers[b] = outliers[s];
        }
    }
    const double *Ps = P + (size_t)s * N * N;
    double *Po = nP + (size_t)b * N * N;
    const long long total = gather_elems(N, lower), pairs = (long long)(N / 2) * (N + 1);
    const long long e0 = (long long)blockIdx.y * GATHER_CHUNK + tid;
    int at[GATHER_UNROLL];
    double v[GATHER_UNROLL];
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u) {
        const long long e = e0 + 256 * u;
        at[u] = -1;
        if (e >= total) continue;
        int idx;
        if (!lower) {
            idx = (int)e;
        } else if (e < pairs) {
            const int qd = (int)(e / (N + 1)), t = (int)(e - (long long)qd * (N + 1));
            int r, c;
            if (t < N - qd) { c = qd; r = qd + t; }                  // column qd, rows qd .. N - 1
            else { c = N - 1 - qd; r = c + (t - (N - qd)); }         // column N - 1 - qd, rows N - 1 - qd .. N - 1
            idx = r + c * N;
        } else {                                                     // odd N: the middle column
            const int c = N / 2;
            idx = c + (int)(e - pairs) + c * N;
        }
        v[u] = Ps[idx];
        at[u] = idx;
    }
#pragma unroll
    for (int u = 0; u < GATHER_UNROLL; ++u)
        if (at[u] >= 0) Po[at[u]] = v[u];
}

#endif // SLK_ENSEMBLE_UNIT

} // namespace slk
