// slk_step_fast.hpp -- exact-shape fast path of the Msckf UKF update with applyDelta (reference src/filters/Msckf.hpp:196-277,
// :400-431, :499-525, :574-589, :659-666, :723-754) for k = 4 .. 8 clones (N = 36 .. 60), m = 8 rows = four 2-D features
// of the registered feature-projection model, 256 threads = four waves per filter.
//
// Same algorithm as msckf_step_kernel's body (slk_kernels.hpp) -- implicit sigma points, S / gate / gain, applyDelta's
// factor as a factor update L' = L chol(I - B B^T), manifold mean with the reference's stop rule, odd / even covariance
// rebuild -- re-laid out so that the hot loops carry no index arithmetic:
//   * the factor lives in LDS as 16 x 16 TILES (tile (I, J) of the lower triangle at (I (I + 1) / 2 + J) * 256, element
//     (t, j) at (j & 15) * 16 + (t & 15), exact zeros above the diagonal and in the padding): every MFMA operand fetch of
//     the factor -- factor update, covariance rebuild -- is `ds_read_b64 base(lane) offset:imm`, conflict free;
//   * one wave per feature evaluates h(X) for the +- pair of a column and the centre point at once (Z_0 by v_readlane, no
//     barrier), S comes from 15 MFMAs on [y+ ; y-] rows, delta = K nu is ONE matrix-vector product L (1/2 dZ S^-1 nu) -- the
//     gain K and covXZ are never formed;
//   * the mean loop works on (block, column) PAIRS: both deviations stay in registers across the convergence test, the
//     first-order correction against the final mean (see slk_kernels.hpp) is applied there, the odd parts go straight into
//     the rotation rows of the tiled factor (so that O = the factor array) and the even parts minus the centre deviation
//     into a k-step-major array E^ in the index space of the rotation rows:
//         P+ = O O^T + E E^T + 1/2 d0 d0^T = O O^T + E^ E^^T + p d0^T + d0 p^T,   p = sum_j e^_j + (N + 1/2) / 2 d0,
//     O and E^ are zero beyond column t + 2 of row t: tile column J of O O^T needs the k-steps 0 .. 4 J + 3 only, one wave
//     per tile column, no cross-wave reduction; E^ E^^T is formed in the rotation-row space (three 16 x 16 tiles, 83 + 37
//     MFMAs at k = 8), takes the rank-2 term (nonzero on rotation rows only) as one more k-step of each tile, and is added
//     where the tiles leave for memory;
//   * tiles leave from the accumulators (mirror triangle) and through a private LDS transpose (lower triangle).
// Anything rare -- failed factorisation, rotation column beyond pi, non-SPD innovation covariance, every block gated out,
// an indefinite downdate, a mean that needs more than 64 rounds, other models / gate modes -- returns false BEFORE the
// first global write and the general body runs instead.
#pragma once
// (included at the end of slk_kernels.hpp: uses its helpers)
#ifdef SLK_STAMPS
#define SLK_FSTAMP(i) do { SLK_STAMP_NR(i); if (a.stop > 0 && a.stop == (i)) return true; } while (0)
#define SLK_WSTAMP(w, i) do { if (tid == 64 * (w) && a.dbg) a.dbg[(size_t)bidx * 32 + (i)] = clock64(); } while (0)
#define SLK_FBAIL(code) do { SLK_NOTE(28, code); return false; } while (0)
#else
#define SLK_FSTAMP(i) do { } while (0)
#define SLK_WSTAMP(w, i) do { } while (0)
#define SLK_FBAIL(code) return false
#endif

// steps between the release B of a staggered plan and the release C under which S and the prefix sums run (fast_release_plan,
// slk_math.hpp; 0: no C, S stays behind the barrier that closes h(X)) -- chosen by A/B, profiles/README.md
#ifndef SLK_RELEASE_HC
#define SLK_RELEASE_HC 3
#endif
// 1: the staggered plan only where it has its release C (A + B alone is behind the single release); 0: wherever two features
// are final three steps ahead of the last one
#ifndef SLK_RELEASE_NEED_C
#define SLK_RELEASE_NEED_C 1
#endif

namespace slk {

// f(FastIdx<I>()) for I = B .. E - 1 while I <= last (wave-uniform, in a scalar register): nested ifs, one scalar compare
// and branch per step, every step its own straight-line code with compile-time indices.  (A `break` in an unrolled loop
// becomes a run-time trip count, the loop stays rolled and its register arrays are indexed at run time.)
template <int I> struct FastIdx { static constexpr int value = I; };
template <int B, int E, class F> __device__ __forceinline__ void fast_steps_to(int last, F &&f)
{
    if constexpr (B < E) {
        if (B <= last) {
            f(FastIdx<B>());
            fast_steps_to<B + 1, E>(last, f);
        }
    }
}

template <int K> struct FastShape {
    static constexpr int N = 12 + 6 * K, Nq = 13 + 7 * K, S = 2 * N + 1, NSO3 = K + 1;
    static constexpr int NT = (N + 15) / 16, NTL = NT * (NT + 1) / 2, NKS = (N + 3) / 4;
    static constexpr int NROT = 3 * NSO3;
    static constexpr int NP = 3 * K * K + 15 * K + 6;          // (block, column) pairs: sum over blocks of toff + 3
    static constexpr int NIT = NP + NSO3;                      // + the centre point of every block (a pair with l = 0)
    static constexpr int RND = (NIT + 255) / 256;
    // LDS carve, doubles
    static constexpr int oLt = 0;                              // tiled factor
    static constexpr int oMu = oLt + NTL * 256;                // mean (Nq)
    static constexpr int oRef = oMu + ((Nq + 7) & ~7);
    static constexpr int oDelta = oRef + ((Nq + 7) & ~7);      // 64
    static constexpr int oMd = oDelta + 64;                    // mean_delta in rotation-row space (32)
    static constexpr int oD0 = oMd + 32;                       // centre deviations (32)
    static constexpr int oD0s = oD0 + 32;                      // (S - 2 (toff + 3)) * centre deviation (32)
    static constexpr int oPd = oD0s + 32;                      // p [32], corrected centre deviations [32]
    static constexpr int oCq = oPd + 64;                       // ref_b^-1 mu_b (4 NSO3 -> 40)
    static constexpr int oStr = oCq + 40;                      // the two odd parts of row 15 that fall into tile (0, 1)
    static constexpr int oInts = oStr + 64;                    // 64 ints
    static constexpr int oTab = oInts + 32;                    // series coefficients (26)
    static constexpr int oMsq = oTab + 28;                     // the two partial sums of |mean_delta|^2 (in the table's unused tail)
    static constexpr int oU = oTab + 32;                       // union region
    // union, phases 1 - 5: Yp [64][17] (rows [y+ ; y-] of a column, one double of padding: the lanes of a wave write
    // different banks; later W [512] and the parked prefix sums), dZ interleaved [512], Sm, mdiag, b, innov, dz0, tmpS
    static constexpr int uYp = 0, uW = 0, uDZ = 1088, uSm = 1600, uMdiag = 1664, uB = 1728, uInnov = 1792, uDz0 = 1800, uTmp = 1808;
    static constexpr int USZ = (NKS * 128 > 1936) ? NKS * 128 : 1936;   // phases 6 - 7: E^ [NKS][2][64]
    static constexpr int total = oU + USZ;
};

static_assert(FastShape<8>::total * 8 * 4 <= 160 * 1024 && FastShape<7>::total * 8 * 4 <= 160 * 1024, "four workgroups per CU");

__host__ __device__ inline int fast_step_lds_doubles(int k)
{
    switch (k) {
    case 4: return FastShape<4>::total;
    case 5: return FastShape<5>::total;
    case 6: return FastShape<6>::total;
    case 7: return FastShape<7>::total;
    case 8: return FastShape<8>::total;
    default: return 0;
    }
}

__device__ __forceinline__ double wave_sum_f64(double x) { return readlane_f64(wave_inclusive_scan(x), 63); }

// rotation-row index (3 b + comp) of tangent row t, 31 (an all-zero row of E^ / p / d0) for vector rows and padding
template <int N> __device__ __forceinline__ int fast_rho(int t)
{
    if (t >= N) return 31;
    if (t < 12) return (t >= 3 && t < 6) ? t - 3 : 31;
    const int cc = (t - 12) / 6, r = (t - 12) - 6 * cc;
    return r >= 3 ? 3 * cc + r : 31;                 // 3 + 3 cc + (r - 3)
}
// storage index of a vector tangent row, -1 for rotation rows (State.hpp:141-149, :246-252, :384-396)
__device__ __forceinline__ int fast_vec_storage(int t)
{
    if (t < 12) return t < 3 ? t : (t < 6 ? -1 : t + 1);
    const int cc = (t - 12) / 6, r = (t - 12) - 6 * cc;
    return r < 3 ? 13 + 7 * cc + r : -1;
}

// ---- SO(3) exp / log with the series coefficients in an LDS table (slk_math.hpp has the same series with literal
// coefficients: inlined a dozen times they pin 26 registers for the whole kernel).  Several arguments are evaluated in
// lockstep so that every coefficient is fetched once.  A wave whose arguments are all small takes the series directly,
// otherwise (uniform branch) an angle-halving form that covers the whole domain the fast path can meet; exp beyond 4 rad
// hands the filter to the general body (flag ints[50], checked after the next barrier, before any global write).
//   T[0..5]   cos sqrt x            degree 6 in y = -x, x <= 1/4   (then 1)     } near-minimax coefficients of
//   T[6..10]  sin sqrt x / sqrt x   degree 5                       (then 1)     } tools/series_coefficients.py (relative
//   T[11..18] atan u / u            degree 8 in y = -u^2, u^2 <= 1/16 (then 1)  } errors 6e-18, 4e-17, 9e-18)
__device__ const double fast_series_table[26] = {
    0x1.1d8d32755f8fbp-29, 0x1.27e40964b47d4p-22, 0x1.a01a00fb1bc6fp-16, 0x1.6c16c16bdd04ep-10, 0x1.5555555555421p-5, 0x1.fffffffffffffp-2,
    0x1.ac53ce336f805p-26, 0x1.71dd113fb7905p-19, 0x1.a01a01061c190p-13, 0x1.11111110ecfb3p-7, 0x1.555555555548fp-3,
    0x1.78be0a9b1dd1fp-5, 0x1.0b3340fe2ed9ap-4, 0x1.3ab708d770276p-4, 0x1.7459b99bfc19bp-4, 0x1.c71c5f4b9c2adp-4, 0x1.24924907fa636p-3, 0x1.999999996d307p-3, 0x1.5555555555481p-2,
    0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

// every active lane's p, as a wave-uniform value: the ballot of !p against zero -- one vector compare and the scalar test
// (__all takes an int: a select and a compare of it on top)
__device__ __forceinline__ bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }

// q[i] = exp(v[i]) for NV rotation vectors.  Rotations below 1 rad (every lane of the wave): the series directly; otherwise
// the series for v / 4 and two quaternion squarings, exp(v) = (exp(v / 4)^2)^2 -- up to 4 rad; ok = false beyond.
// Two code paths behind the uniform branch, the series written out in each: merged into one with the halving selected in,
// every call pays both squarings and six selects per argument.  The domain tests x < 1/4, x < 4 are taken on the largest
// upper dword of the x (nonneg_hi_below, slk_math.hpp: x is a scaled sum of squares), the second on the halved path only
// (x < 1/4 implies it).
template <int NV, bool WIDE>
__device__ __forceinline__ void so3_exp_tab_path(const double *T, const double (&v)[NV][3], const double (&x)[NV], Quat (&q)[NV])
{
    double y[NV], cc[NV], ss[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) y[i] = WIDE ? -0.0625 * x[i] : -x[i];   // wide: |v / 4|^2 / 4
    {
        const double c0 = T[0], s0 = T[6];
#pragma unroll
        for (int i = 0; i < NV; ++i) { cc[i] = c0; ss[i] = s0; }
    }
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const double ck = T[k], sk = T[6 + k];
#pragma unroll
        for (int i = 0; i < NV; ++i) { cc[i] = fma(cc[i], y[i], ck); ss[i] = fma(ss[i], y[i], sk); }
    }
    {
        const double c5 = T[5];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            cc[i] = fma(cc[i], y[i], c5);
            cc[i] = fma(cc[i], y[i], 1.0);
            ss[i] = fma(ss[i], y[i], 1.0);
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double m = 0.5 * ss[i], w = cc[i];           // exp(v) = (m v, w);  wide: exp(v / 4) = (m / 4 v, w)
        if (WIDE) {
            m *= 0.25;
#pragma unroll
            for (int rep = 0; rep < 2; ++rep) {      // (w, m v)^2 = (2 w^2 - 1, 2 w m v) for a unit quaternion
                const double w2 = fma(2.0 * w, w, -1.0);
                m = 2.0 * w * m;
                w = w2;
            }
        }
        q[i] = Quat{m * v[i][0], m * v[i][1], m * v[i][2], w};
    }
}
// FLAG: an argument beyond 4 rad in any lane sets *flag where it is found, on the halved path (the result is true then);
// else the lane's own ok is the result
template <int NV, bool FLAG>
__device__ __forceinline__ bool so3_exp_tab_impl(const double *T, const double (&v)[NV][3], Quat (&q)[NV], int *flag)
{
    double x[NV];
    unsigned hm = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        x[i] = 0.25 * (v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2]);
        const unsigned hi = (unsigned)__double2hiint(x[i]);
        hm = hi > hm ? hi : hm;
    }
    if (wave_all(nonneg_hi_below(hm, HI_QUARTER))) { // (uniform over the wave)
        so3_exp_tab_path<NV, false>(T, v, x, q);
        return true;
    }
    so3_exp_tab_path<NV, true>(T, v, x, q);
    const bool ok = nonneg_hi_below(hm, HI_FOUR);
    if (!FLAG) return ok;
    if (!wave_all(ok)) *flag = 1;
    return true;
}
// a * b for b = an exponential of so3_exp_tab: qmul's products and sums with the contraction written out, from the left.  Left
// to the compiler, which of the two products of `a.w * b.x + a.x * b.w` is rounded before the other is fused onto it depends on
// where b.w comes from (one code path or two): one rounding per component that moved with the code around it.
__device__ __forceinline__ Quat qmul_exp(const Quat &a, const Quat &b)
{
    Quat o;
    o.w = fma(-a.z, b.z, fma(-a.y, b.y, fma(a.w, b.w, -(a.x * b.x))));
    o.x = fma(-a.z, b.y, fma(a.y, b.z, fma(a.x, b.w, a.w * b.x)));
    o.y = fma(-a.x, b.z, fma(a.z, b.x, fma(a.y, b.w, a.w * b.y)));
    o.z = fma(-a.y, b.x, fma(a.x, b.y, fma(a.z, b.w, a.w * b.z)));
    return o;
}
template <int NV>
__device__ __forceinline__ bool so3_exp_tab(const double *T, const double (&v)[NV][3], Quat (&q)[NV])
{
    return so3_exp_tab_impl<NV, false>(T, v, q, nullptr);
}
template <int NV>
__device__ __forceinline__ void so3_exp_tab_flag(const double *T, const double (&v)[NV][3], Quat (&q)[NV], int *flag)
{
    so3_exp_tab_impl<NV, true>(T, v, q, flag);
}
// d[i] = log(q[i]) in MTK's form 2 atan(|vec| / w) / |vec| * vec (q and -q give the same result).  Rotations below ~28
// degrees (every lane of the wave): the series of atan(u) / u directly, u = |vec| / w.  Otherwise by halved angles:
// with w >= 0 (else take -q), t1 = tan(theta / 4) = |vec| / (1 + w) <= 1, two more halvings t <- t / (1 + sqrt(1 + t^2))
// bring tan(theta / 16) below 0.2, theta = 16 atan(t3): every unit quaternion is inside this domain.
template <int NV>
__device__ __forceinline__ bool so3_log_tab(const double *T, const Quat (&q)[NV], double (&d)[NV][3])
{
    double y[NV], sc[NV], f[NV];
    bool small = true;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        // w > 0 and 16 n2 < w^2 in one compare: w |w| is w^2 with the sign of w (the same product, the same rounding), and
        // 16 n2 >= +0 is below nothing that is negative, a zero or a NaN
        const double n2 = q[i].x * q[i].x + q[i].y * q[i].y + q[i].z * q[i].z, ws = q[i].w * fabs(q[i].w);
        small = small && (n2 * 16.0 < ws);
        y[i] = n2;
    }
    const bool wide = !wave_all(small);              // (uniform over the wave)
    if (!wide) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const double r = rcp_refined(q[i].w);
            sc[i] = 2.0 * r;                         // log(q) = 2 / w * [atan(u) / u] * vec
            y[i] = -(y[i] * r * r);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const double n2 = y[i], aw = fabs(q[i].w);
            const double r = rcp_refined(1.0 + aw);
            double k = r, t2 = n2 * r * r;           // tan(theta / 4) = k |vec|, its square
#pragma unroll
            for (int rep = 0; rep < 2; ++rep) {      // t <- t / (1 + sqrt(1 + t^2))
                const double a1 = 1.0 + t2;
                double sq, rs;
                rsqrt_pivot(a1, sq, rs);
                const double den = fma(a1, rs, 1.0);  // 1 + sqrt(1 + t^2)
                const double rd = rcp_refined(den);
                k *= rd;
                t2 *= rd * rd;
            }
            sc[i] = (q[i].w < 0.0) ? -16.0 * k : 16.0 * k;   // theta / |vec| = 16 atan(t3) / |vec| = 16 k [atan(t3) / t3]
            y[i] = -t2;
        }
    }
    {
        const double a0 = T[11];
#pragma unroll
        for (int i = 0; i < NV; ++i) f[i] = a0;
    }
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const double ak = T[11 + k];
#pragma unroll
        for (int i = 0; i < NV; ++i) f[i] = fma(f[i], y[i], ak);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        f[i] = fma(f[i], y[i], 1.0);
        const double sv = sc[i] * f[i];
        d[i][0] = sv * q[i].x; d[i][1] = sv * q[i].y; d[i][2] = sv * q[i].z;
    }
    return true;
}

// The factor update needs, for every column j, 4 G_j = sum_{k < j} dZ_k dZ_k^T (8 x 8 symmetric; ldm_prefix of slk_kernels.hpp
// takes the 36 entries from 36 wave scans).  Here in BLOCKS of four columns, block b = columns 4 b .. 4 b + 3:
//   * fast_prefix_blocks: one wave runs acc <- mfma(fr, fr, acc) over the k-steps, fr = rows (c16 & 7) of dZ at column
//     4 s + g (rows / columns 8 .. 15 of the tile repeat 0 .. 7 and are never read): after step s the top-left 8 x 8 of acc is
//     the BASE 4 G_{4 (s + 1)} of block s + 1.  Lane (c16, g) holds rows g and g + 4 of column c16, and the lanes c16 >= 8
//     the same numbers as the lanes c16 - 8: the lower half of the lanes keeps row g, the upper half row g + 4 -- ONE double
//     per step and lane, in registers (no LDS is free while S is formed) until fast_prefix_park puts them, one full-wave
//     store per step, into NKS slots of an 8 x 8 each (slot 0 = zeros), kPrefixSlot doubles apart: the sixteen blocks of a
//     wave's lanes then read sixteen different banks.
//   * fast_prefix_tail: lane j = column j sums the outer products of the up-to-three columns before it INSIDE its block; a
//     neighbour outside the block is replaced by column 63 of dZ, which is exactly zero for every N <= 60 (an integer
//     select on the address, none on values).
//   * lane j's 4 G_j = slot[min(j >> 2, NKS - 1)] + tail.  The clamp is the dead-lane rule: fast_ldm_columns tests d > 0 over
//     all 64 lanes, so lanes j >= N need a T_j that is positive definite -- theirs is that of a live column (columns >= N of dZ
//     are zero: a dead lane inside the last block has the true prefix, one beyond it G of that block's first column).
//   * the columns beyond jmax (the last one a measurement row depends on) of dZ are exact zeros: the steps of the chain
//     beyond ksmax = jmax >> 2 add +0 and leave the sum over all live columns, bit for bit, in every later base.  So only
//     min(ksmax + 2, NKS) slots are parked and the slot index is clamped to ksmax + 1 as well (fast_prefix_slot): every
//     block behind the last live one reads that sum from the first slot that holds it.  (The chain itself runs all its
//     steps, see there.)
// The factor 1/4 (a = 1/2 dZ) is a power of two and goes into T = S - 1/4 (4 G) of fast_ldm_columns, exactly.
// All of it runs on the wave that consumes it (wave 3; chain and tails beside S, where that wave was idle): the slots are
// written and read by one wave, and the step has one barrier less than with the sums handed over from another wave.
constexpr int kPrefixSlot = 66;
template <int NKS>
__device__ __forceinline__ void fast_prefix_blocks(const double *dZi, int c16, int g4, double (&Gs)[NKS - 1])
{
    static_assert(NKS * kPrefixSlot <= 1088, "block bases: the dead Yp rows");
    const double *fp = dZi + ((c16 & 7) >> 1) * 128 + 2 * g4 + (c16 & 1);
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    // (all NKS - 1 steps, also those beyond the last live one that add exact zeros: with a uniform exit per step, or per two
    // steps, the chain is no longer one block, the operand fetch and its address stay live beside the 36 tails and the 14
    // bases, and the k = 8 kernel spills 8 to 12 registers)
#pragma unroll
    for (int s = 0; s < NKS - 1; ++s) {
        const double fr = fp[8 * s];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fr, fr, acc, 0, 0, 0);
        Gs[s] = (c16 < 8) ? acc[0] : acc[1];
    }
}
template <int NKS>
__device__ __forceinline__ void fast_prefix_park(double *slots, int c16, int g4, int ksmax, const double (&Gs)[NKS - 1])
{
    double *sp = slots + 8 * (c16 & 7) + g4 + 4 * (c16 >> 3);
    sp[0] = 0.0;
    fast_steps_to<0, NKS - 1>(ksmax, [&](auto ix) __attribute__((always_inline)) {
        constexpr int s = decltype(ix)::value;
        sp[(s + 1) * kPrefixSlot] = Gs[s];
    });
}
// the slot of lane j's block: its own up to the one behind the last live k-step, whose base is the sum over every live column
__device__ __forceinline__ int fast_prefix_slot(int j, int ksmax, int nks)
{
    const int last = ksmax + 1 < nks - 1 ? ksmax + 1 : nks - 1;
    const int blk = j >> 2;
    return blk < last ? blk : last;
}
__device__ __forceinline__ void fast_prefix_tail(const double *dZi, int lane, double (&Gs)[36])
{
    const double2 *dz2 = reinterpret_cast<const double2 *>(dZi);
    const int q = lane & 3;
#pragma unroll
    for (int n = 1; n <= 3; ++n) {
        const int cn = (q >= n) ? lane - n : 63;
        double v[8];
#pragma unroll
        for (int p = 0; p < 4; ++p) { const double2 t = dz2[p * 64 + cn]; v[2 * p] = t.x; v[2 * p + 1] = t.y; }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
#pragma unroll
            for (int cc = 0; cc <= r; ++cc) {
                const int e = r * (r + 1) / 2 + cc;
                Gs[e] = (n == 1) ? v[r] * v[cc] : fma(v[r], v[cc], Gs[e]);
            }
        }
    }
}

// (block, column) pairs of the mean loop, tabulated at compile time: one 64-bit word per pair
//   low dword : bits 0-12 / 13-25 offsets (doubles, from the start of LDS) of L'(toff, j) / L'(toff + 1, j) (an always-zero
//               element where the tile is not stored), 26-29 the SO(3) block, 30-31 1 / 2 = the odd part of component 0 goes
//               to str[15] / str[31] (row 15's columns 16 / 17, whose tile (0, 1) is not stored)
//   high dword: bits 0-12 offset of L'(toff + 2, j), 13-23 offset of component 0 in E^
template <int K> struct FastPairTable {
    unsigned long long v[FastShape<K>::NP];
    constexpr FastPairTable() : v{}
    {
        int p = 0;
        for (int b = 0; b <= K; ++b) {
            const int to = b ? 9 + 6 * b : 3;
            for (int j = 0; j < to + 3; ++j, ++p) {
                unsigned long long a[3] = {0, 0, 0};
                for (int cc = 0; cc < 3; ++cc) {
                    const int t = to + cc, I = t >> 4, Jc = j >> 4;
                    a[cc] = (unsigned long long)(FastShape<K>::oLt + (Jc <= I ? (I * (I + 1) / 2 + Jc) * 256 + (j & 15) * 16 + (t & 15) : 16));
                }
                const int rho = 3 * b;
                const unsigned long long e0 = (unsigned long long)(((j >> 2) * 2 + (rho >> 4)) * 64 + (j & 3) * 16 + (rho & 15));
                const unsigned long long sd = (b == 1 && j >= 16) ? (unsigned long long)(j - 15) : 0ull;
                v[p] = a[0] | (a[1] << 13) | ((unsigned long long)b << 26) | (sd << 30) | (a[2] << 32) | (e0 << 45);
            }
        }
    }
};
template <int K> struct FastPairTableHolder { static __device__ const FastPairTable<K> tab; };
template <int K> __device__ const FastPairTable<K> FastPairTableHolder<K>::tab = FastPairTable<K>();

// ldm_columns (slk_kernels.hpp) with the column's deviations a_j = 1/2 dZ_j fetched from LDS where they are used instead of
// held in sixteen registers beside the 36 prefix sums: lane j = column j, Gf + bp[8 c + r] = 4 G_j = the prefix sums of
// dZ dZ^T (tail + the 8 x 8 base of the lane's block, see fast_prefix_blocks; the base is fetched and the 1/4 applied where
// column c of T_j = S - G_j is formed: all 36 bases fetched ahead spill), Sm = S (8 x 8), kept = rows that survived the gate.  Writes Wb[bw_idx(j, :)] = 1/2 w~_j and mdiag[j] = sqrt(d_j); false if Pk - K S K^T is not
// positive definite.
#define SLK_G(r, c) Gf[(r) * ((r) + 1) / 2 + (c)]
__device__ __forceinline__ bool fast_ldm_columns(double (&Gf)[36], const double *bp, const double *dZi, const double *Sm, unsigned kept, int lane, int N,
                                                 double *Wb, double *mdiag)
{
    const bool live = lane < N;
    // set-up: T_j = S - G_j over the surviving rows, identity rows for the rejected ones -- column j of it at step j of the
    // chain below, where it is first read.  kept is wave-uniform and nearly always 0xff: that case takes the plain loads and
    // subtractions (no select, no select-addressed LDS read per entry) behind a uniform branch; the chain itself is ONE copy
    // of code.  (All 36 entries set up ahead of the chain in two forms: the kernel spills -- 44 registers, 128 B of scratch.)
    const bool full = kept == 0xffu;
    // T_j = R R^T in place (R lower, its diagonal kept as reciprocals), y = R^-1 b, d = 1 - |y|^2, w = -R^-T y / sqrt(d)
    double y[8];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (full) {
#pragma unroll
            for (int r = j; r < 8; ++r) SLK_G(r, j) = fma(-0.25, bp[8 * j + r] + SLK_G(r, j), Sm[r + 8 * j]);
        } else {
            const bool kj = (kept >> j) & 1u;
#pragma unroll
            for (int r = j; r < 8; ++r) {
                const bool in = kj && ((kept >> r) & 1u);
                const double sv = Sm[in ? r + 8 * j : 0];
                SLK_G(r, j) = in ? fma(-0.25, bp[8 * j + r] + SLK_G(r, j), sv) : ((r == j) ? 1.0 : 0.0);
            }
        }
        double d = SLK_G(j, j);
#pragma unroll
        for (int p = 0; p < j; ++p) d = fma(-SLK_G(j, p), SLK_G(j, p), d);
        ok = ok && (d > 0.0);
        double sq, rs;
        rsqrt_pivot(d, sq, rs);
        SLK_G(j, j) = rs;
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
            double v = SLK_G(i, j);
#pragma unroll
            for (int p = 0; p < j; ++p) v = fma(-SLK_G(i, p), SLK_G(j, p), v);
            SLK_G(i, j) = v * rs;
        }
        const double aj = dZi[(j >> 1) * 128 + 2 * lane + (j & 1)];
        double sacc = ((kept >> j) & 1u) ? 0.5 * aj : 0.0;
#pragma unroll
        for (int p = 0; p < j; ++p) sacc = fma(-SLK_G(j, p), y[p], sacc);
        y[j] = sacc * rs;
    }
    double dj = 1.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) dj = fma(-y[c], y[c], dj);
    ok = ok && (dj > 0.0);
    double sqd, rsd;
    rsqrt_pivot(dj, sqd, rsd);
    const double sc = -0.5 * rsd;
#pragma unroll
    for (int c = 7; c >= 0; --c) {                   // w overwrites y from the back
        double sacc = y[c];
#pragma unroll
        for (int p = c + 1; p < 8; ++p) sacc = fma(-SLK_G(p, c), y[p], sacc);
        y[c] = sacc * SLK_G(c, c);
        Wb[bw_idx(lane, c)] = live ? y[c] * sc : 0.0;
    }
    mdiag[lane] = live ? sqd : 1.0;
    return __all(ok) != 0;
}
#undef SLK_G

// Output tile (I, J) of the factor update -> the wave that computes it.  The tiles of one tile column share their M tiles
// M(Kb, J) = dZ_Kb W_J^T (2 MFMAs each, formed once per wave and tile column; 4 more per (tile, Kb) for the product with
// L(I, Kb)), so the map keeps tile columns together: the one with the fewest MFMAs in all among those whose longest wave is
// no longer than under ldm_tile_wave (slk_kernels.hpp: 30 at NT = 4, 18 at NT = 3) -- tools/ldm_tile_assignment.py.
// MFMAs per wave, JB = the last tile column that is not skipped:
//   NT = 4   wave 0: (3,0) (0,0)   wave 1: (2,0) (1,0)   wave 2: (3,1) (2,1) (1,1)   wave 3: (3,2) (2,2) (3,3)
//            JB = 3: 28 / 26 / 30 / 22 = 106 (ldm_tile_wave: 4 x 30)     JB = 2 (the benchmark): 22 / 26 / 24 / 10 = 82 (4 x 24)
//            JB = 1: 16 / 20 / 14 / 0                                    JB = 0: 10 / 10 / 0 / 0
//   NT = 3   wave 0: (1,0) (0,0)   wave 1: (2,1) (1,1)   wave 2: (2,0)   wave 3: (2,2)
//            JB = 2: 16 / 16 / 18 / 6 = 56 (18 / 18 / 18 / 6)            JB = 1: 16 / 10 / 12 / 0     JB = 0: 10 / 0 / 6 / 0
// These are the counts with jmax (the last column a measurement row depends on) at the end of tile column JB, for which the
// map is chosen.  Below the diagonal the k-steps of M(Kb, J) beyond jmax are dropped as well (fast_ldm_wave_tiles): at
// jmax = 35 (the benchmark: tile row 2 has one live k-step of four) NT = 4 runs 19 / 23 / 18 / 10 = 70, NT = 3 (k = 5, 6)
// 16 / 13 / 15 / 6 = 50.
template <int NT> __host__ __device__ constexpr int fast_ldm_wave(int I, int J)
{
    if (NT == 4) return J == 0 ? ((I == 3 || I == 0) ? 0 : 1) : (J == 1 ? 2 : 3);
    return J == 0 ? (I == 2 ? 2 : 0) : (J == 1 ? 1 : 3);
}
// position of tile (I, J) among the tiles of its wave: a compile-time accumulator index
template <int NT> __host__ __device__ constexpr int fast_ldm_slot(int I, int J)
{
    int n = 0;
    for (int i = 0; i < NT; ++i)
        for (int j = 0; j <= i; ++j) {
            if (i == I && j == J) return n;
            if (fast_ldm_wave<NT>(i, j) == fast_ldm_wave<NT>(I, J)) ++n;
        }
    return n;
}
// does wave W own a tile (I, J) with I >= K0
template <int NT> __host__ __device__ constexpr bool fast_ldm_owns(int W, int J, int K0)
{
    for (int i = (K0 > J ? K0 : J); i < NT; ++i)
        if (fast_ldm_wave<NT>(i, J) == W) return true;
    return false;
}

// the tiles of wave W: every M(Kb, J) once, then into each of the wave's tiles (I, J), I >= Kb -- per output element the
// operations and their order (Kb ascending from J) of one tile at a time.  Below the diagonal (Kb > J) the rows k > jmax of
// M(Kb, J) are a_k w~^T = 0 exactly, so the product with L(I, Kb) runs its k-steps (four rows each) only while
// 16 Kb + 4 s <= jmax, a uniform exit, and fetches only those fragments of L; a diagonal tile keeps all four (its rows
// beyond jmax are identity rows, which copy L's columns).
template <int NT, int W, int MAXT>
__device__ __forceinline__ void fast_ldm_wave_tiles(const double *Lt, const double *dZi, const double *Wb, const double *mdiag, int lane,
                                                    int jmax, d4 (&acc)[MAXT])
{
    const int JB = jmax >> 4;
    const int c = lane & 15, g = lane >> 4;
    const int lw = (g >> 1) * 128 + 2 * c + (g & 1);           // lane part of bw_idx(16 X + c, g)
#pragma unroll
    for (int J = 0; J < NT; ++J) {
        if (!fast_ldm_owns<NT>(W, J, J) || J > JB) continue;
        const double wf0 = Wb[32 * J + lw], wf1 = Wb[256 + 32 * J + lw];
#pragma unroll
        for (int Kb = J; Kb < NT; ++Kb) {
            if (!fast_ldm_owns<NT>(W, J, Kb) || Kb > JB) continue;
            const int slast = (Kb > J) ? (jmax - 16 * Kb) >> 2 : 3;   // the last k-step of M(Kb, J) with a row <= jmax (Kb <= JB: >= 0)
            d4 mt = {0.0, 0.0, 0.0, 0.0};
            const double a0 = dZi[32 * Kb + lw], a1 = dZi[256 + 32 * Kb + lw];
            mt = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, wf0, mt, 0, 0, 0);
            mt = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, wf1, mt, 0, 0, 0);
            if (Kb == J) {
                const double dg = mdiag[16 * J + c];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = g + 4 * r;
                    mt[r] = (row > c) ? mt[r] : ((row == c) ? dg : 0.0);
                }
            }
#pragma unroll
            for (int I = Kb; I < NT; ++I) {
                if (fast_ldm_wave<NT>(I, J) != W) continue;
                double lf[4];
                const double *lp = Lt + (I * (I + 1) / 2 + Kb) * 256 + lane;
                fast_steps_to<0, 4>(slast, [&](auto ix) __attribute__((always_inline)) {
                    constexpr int s = decltype(ix)::value;
                    lf[s] = lp[64 * s];
                });
                d4 &a = acc[fast_ldm_slot<NT>(I, J)];
                fast_steps_to<0, 4>(slast, [&](auto ix) __attribute__((always_inline)) {
                    constexpr int s = decltype(ix)::value;
                    a = __builtin_amdgcn_mfma_f64_16x16x4f64(mt[s], lf[s], a, 0, 0, 0);
                });
            }
        }
    }
}

// L <- L M on the matrix cores, tiled factor (see ldm_product in slk_kernels.hpp for the algebra).  jmax = the last column
// any measurement row depends on, JB = its tile column: beyond it M is the identity (dZ rows are exactly zero), those blocks
// are skipped, and so are the k-steps beyond jmax below the diagonal (fast_ldm_wave_tiles).  fill() runs between the two
// barriers (everything but the factor is dead there).
template <int NT, class FillFn>
__device__ __forceinline__ void ldm_product_tiled(double *Lt, const double *dZi, const double *Wb, const double *mdiag, int lane,
                                                  int wave, int jmax, FillFn fill)
{
    constexpr int MAXT = (NT == 4) ? 3 : 2;
    const int JB = jmax >> 4;
    d4 acc[MAXT];
#pragma unroll
    for (int q = 0; q < MAXT; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    if (wave == 0) fast_ldm_wave_tiles<NT, 0>(Lt, dZi, Wb, mdiag, lane, jmax, acc);
    else if (wave == 1) fast_ldm_wave_tiles<NT, 1>(Lt, dZi, Wb, mdiag, lane, jmax, acc);
    else if (wave == 2) fast_ldm_wave_tiles<NT, 2>(Lt, dZi, Wb, mdiag, lane, jmax, acc);
    else fast_ldm_wave_tiles<NT, 3>(Lt, dZi, Wb, mdiag, lane, jmax, acc);
    __syncthreads();                                  // every wave has read what it needs of the old factor
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J <= I; ++J) {
            if (fast_ldm_wave<NT>(I, J) != wave || J > JB) continue;
            const d4 a = acc[fast_ldm_slot<NT>(I, J)];
#pragma unroll
            for (int r = 0; r < 4; ++r) Lt[(I * (I + 1) / 2 + J) * 256 + 64 * r + lane] = a[r];
        }
    fill();
    __syncthreads();
}

// The even-part product EE = E^ E^^T in the index space of the rotation rows, where E^ is stored: 32 x 32 (27 rows at k = 8),
// three lower 16 x 16 tiles (one when every rotation row is below 16, k = 4).  Row rho of E^ is zero beyond column
// toff(block) + 2, which bounds the k-steps of the tiles with rows below 16.  The result goes to LDS as a full symmetric
// matrix ee[32][EES] (padding rows / columns exact zeros) and is added where the tiles of P+ leave for memory.
template <int K> struct FastEE {
    using F = FastShape<K>;
    static constexpr int EES = 40;                               // row stride: rows g, g + 1 of a store land 16 banks apart
    static constexpr int NTE = F::NROT > 16 ? 2 : 1;
    static constexpr int PAD = 16 * NTE - 1;                     // an all-zero row / column of E^ inside the published tiles
    static constexpr int BLO = F::NSO3 - 1 < 5 ? F::NSO3 - 1 : 5;   // last block with a row below 16 (rho = 3 b)
    static constexpr int CLO = (BLO ? 9 + 6 * BLO : 3) + 3;      // its columns end here
    static constexpr int KS0 = ((CLO + 3) / 4 < F::NKS) ? (CLO + 3) / 4 : F::NKS;   // k-steps of the tiles (0, 0), (1, 0)
    static constexpr int KS1 = F::NKS;                           // ... of tile (1, 1)
    // the wave of a tile: the O part gives the waves 20 / 24 / 24 / 15 MFMAs at k = 8 and wave 1 has the second round of
    // the mean loop, so (0, 0) -> wave 0, (1, 0) -> wave 2, (1, 1) -> wave 3
    __host__ __device__ static constexpr int wave_of(int hi, int hj) { return hi == 0 ? 0 : (hj == 0 ? 2 : 3); }
};
static_assert(32 * FastEE<8>::EES <= FastShape<4>::USZ, "EE fits the union region");

// tile (HI, HJ) of EE from the fragments of E^: a row-rho fragment of k-step ks is Et[ks * 128 + (rho >> 4) * 64 + lane]
template <int K, int HI, int HJ>
__device__ __forceinline__ d4 fast_ee_tile(const double *Et, int lane)
{
    constexpr int KE = HJ == 0 ? FastEE<K>::KS0 : FastEE<K>::KS1;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KE; ++ks) {
        const double fj = Et[ks * 128 + HJ * 64 + lane];
        const double fi = HI == HJ ? fj : Et[ks * 128 + HI * 64 + lane];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fi, fj, acc, 0, 0, 0);
    }
    return acc;
}
// ... + p d0^T + d0 p^T, the rank-2 term of P+, which lives on the rotation rows as well: one more k-step of the tile,
// A = [p, d0, 0, 0], B = [d0, p, 0, 0] (pd = p [32], d0 [32]; rows from NROT on, pd[31] among them, are exact zeros)
template <int HI, int HJ>
__device__ __forceinline__ d4 fast_ee_rank2(const double *pd, int lane, const d4 &acc)
{
    const int c = lane & 15, g = lane >> 4;
    const double af = pd[g == 0 ? 16 * HI + c : (g == 1 ? 32 + 16 * HI + c : 31)];
    const double bf = pd[g == 0 ? 32 + 16 * HJ + c : (g == 1 ? 16 * HJ + c : 31)];
    return __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc, 0, 0, 0);
}
// acc[r] of lane (c, g) = EE(16 HI + g + 4 r, 16 HJ + c); an off-diagonal tile in both orientations
template <int K, int HI, int HJ>
__device__ __forceinline__ void fast_ee_publish(double *ee, int lane, const d4 &acc)
{
    constexpr int EES = FastEE<K>::EES;
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ee[(16 * HI + g + 4 * r) * EES + 16 * HJ + c] = acc[r];
        if (HI != HJ) ee[(16 * HJ + c) * EES + 16 * HI + g + 4 * r] = acc[r];
    }
}

// rotation-row indices of the tangent rows 16 I + G + 4 r (r = 0 .. 3), one byte each (PAD, an all-zero row of EE, for
// vector rows and padding): the rows a lane of group G = lane >> 4 holds in the accumulator of a tile of row block I
template <int K> __host__ __device__ constexpr unsigned fast_rho_pack(int I, int G)
{
    constexpr int N = FastShape<K>::N, PAD = FastEE<K>::PAD;
    unsigned w = 0;
    for (int r = 0; r < 4; ++r) {
        const int t = 16 * I + G + 4 * r;
        int rho = PAD;
        if (t < N) {
            if (t < 12) rho = (t >= 3 && t < 6) ? t - 3 : PAD;
            else { const int cc = (t - 12) / 6, q = (t - 12) - 6 * cc; rho = q >= 3 ? 3 * cc + q : PAD; }
        }
        w |= (unsigned)rho << (8 * r);
    }
    return w;
}

// One tile column J of O O^T (k-steps 0 .. 4 J + 3; tile column 0 also the step that holds row 15's columns 16 / 17):
// acc[I - J] += frag(I) frag(J)^T.
template <int K, int J>
__device__ __forceinline__ void fast_rebuild_col(const double *Lt, const double *str, int lane, d4 (&acc)[FastShape<K>::NT])
{
    using F = FastShape<K>;
    constexpr int NT = F::NT;
    constexpr int KEND = (4 * J + 4 + (J == 0 ? 1 : 0) < F::NKS) ? 4 * J + 4 + (J == 0 ? 1 : 0) : F::NKS;
#pragma unroll
    for (int ks = 0; ks < KEND; ++ks) {
        double fo[NT];
#pragma unroll
        for (int I = J; I < NT; ++I) {
            const int Kc = ks >> 2;
            fo[I] = (Kc <= I) ? Lt[(I * (I + 1) / 2 + Kc) * 256 + (ks & 3) * 64 + lane] : str[lane];
        }
#pragma unroll
        for (int I = J; I < NT; ++I) acc[I - J] = __builtin_amdgcn_mfma_f64_16x16x4f64(fo[I], fo[J], acc[I - J], 0, 0, 0);
    }
}

// Out: the mirror triangle straight from the accumulators, the lower triangle of the off-diagonal tiles through a private
// 16 x 17 transpose buffer.
// Before either store every element takes its share of the even-part product and the rank-2 term (fast_ee_rank2),
// P+(t, s) += EE(rho(t), rho(s)) (vector rows and columns read an exact zero): both orientations carry the same sum.
template <int K, int J>
__device__ __forceinline__ void fast_store_col(const double *ee, double *bufs, double *oP, int lane, d4 (&acc)[FastShape<K>::NT],
                                               bool lower_only)
{
    using F = FastShape<K>;
    constexpr int NT = F::NT, N = F::N, EES = FastEE<K>::EES, PAD = FastEE<K>::PAD;
    const int c = lane & 15, g = lane >> 4;
    {
        const int rj = fast_rho<N>(16 * J + c);
        const double *eec = ee + (rj & PAD);                     // (31 & PAD = PAD)
#pragma unroll
        for (int I = J; I < NT; ++I) {
            const unsigned rw = g == 0 ? fast_rho_pack<K>(I, 0) : (g == 1 ? fast_rho_pack<K>(I, 1) : (g == 2 ? fast_rho_pack<K>(I, 2) : fast_rho_pack<K>(I, 3)));
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[I - J][r] += eec[((rw >> (8 * r)) & 0xffu) * EES];
        }
    }
    double *o = oP + c + g * N;                      // lane part of both orientations
#pragma unroll
    for (int I = J; I < NT; ++I) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {                // acc[r] of lane (c, g) = P+(16 I + g + 4 r, 16 J + c) -> P(col, row)
            const bool full = 16 * I + 4 * r + 3 < N && 16 * J + 15 < N;
            if (I > J && lower_only) continue;       // (the mirror triangle is brought up to date when somebody wants it)
            if (16 * I + 4 * r < N && (full || (16 * I + 4 * r + g < N && 16 * J + c < N)))
                o[16 * J + (16 * I + 4 * r) * N] = acc[I - J][r];
        }
        if (I > J) {
            double *buf = bufs + (I * (I - 1) / 2 + J) * 272;
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[c * 17 + g + 4 * r] = acc[I - J][r];     // buf[col][row]
            wave_sync();
#pragma unroll
            for (int q = 0; q < 4; ++q) {            // lane (c, g): row 16 I + c, column 16 J + g + 4 q
                const double v = buf[(g + 4 * q) * 17 + c];
                const bool full = 16 * I + 15 < N;   // (columns of an off-diagonal tile are always inside)
                if (full || 16 * I + c < N) o[16 * I + (16 * J + 4 * q) * N] = v;
            }
        }
    }
}

template <int K>
__device__ __forceinline__ bool msckf_step_fast(const KArgs &a, double *smem)
{
    using F = FastShape<K>;
    constexpr int N = F::N, Nq = F::Nq, S = F::S, NSO3 = F::NSO3, NT = F::NT, NKS = F::NKS, NROT = F::NROT;
    constexpr int NP = F::NP;
    constexpr int NTHREADS = 256;                                // four waves (HasFastStep: the only block size that gets here)
    if (a.mm != SLK_MM_FEATURE_PROJ || a.gate == 2 || a.emit != 0 || a.rebuild_prec != 0 || !a.mp || a.m != 8) return false;
    const int bidx = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g4 = lane >> 4;
    double *Lt = smem + F::oLt, *mu = smem + F::oMu, *ref = smem + F::oRef, *delta = smem + F::oDelta, *md32 = smem + F::oMd;
    double *d0 = smem + F::oD0, *d0s = smem + F::oD0s, *pd = smem + F::oPd, *cq = smem + F::oCq, *str = smem + F::oStr, *U = smem + F::oU;
    int *ints = reinterpret_cast<int *>(smem + F::oInts);          // [0..39] gate lists of the waves, [48] [49] flags
    double *T = smem + F::oTab, *msq = smem + F::oMsq;
    double *Yp = U + F::uYp, *Wb = U + F::uW, *dZi = U + F::uDZ, *Sm = U + F::uSm, *mdiag = U + F::uMdiag, *bvec = U + F::uB;
    double *innov = U + F::uInnov, *dz0 = U + F::uDz0, *tmpS = U + F::uTmp, *Et = U;
    const double *gmean = a.mean + (size_t)bidx * Nq;
    const double *gP = a.P + (size_t)bidx * N * N;
    const double *mp = a.mp + (size_t)bidx * a.mp_stride;
    SLK_STAMP_NR(0);

    // ---- phase 0: mean, tiled factor, small arrays.  Every global load is issued before the first use; the conditions that
    // hand the filter to the general body -- failed first factorisation, pose index out of range (SLK_ST_BAD_INDEX there),
    // a rotation column that may exceed pi (Msckf.hpp:407-413: covXZ = L A would not hold) -- meet in one barrier
    // jmax = the last column any measurement row depends on (a feature on pose c reaches the columns j <= tp + 5: the lanes
    // beyond evaluate X_0, y+ = y- = 0 and dZ_j = 0 exactly), ksmax = jmax >> 2 = the last k-step (four columns) with a live
    // column, both wave-uniform and held in scalar registers.  S, the block bases of the prefix sums, delta = L b and the
    // k-blocks below the diagonal of the factor update stop there: what lies beyond multiplies exact zeros.
    int jmax = 0, ksmax, bad;
    FastReleasePlan plan;
    // the factor: from msckf_chol_kernel's workspace, or (a.wsfail == nullptr) factored HERE by wave 0 -- cholp_factor, panel
    // by rows, straight into the tiles -- while the other waves fetch the small arrays (against the factor through the
    // workspace for every step: same step time, 0.74 x instead of 1.28 x the algorithmic bytes,
    // profiles/r03_ab_msckf_factor_inside.log)
    const bool here = a.wsfail == nullptr;
    {
        const double *gL = here ? gP : a.wsL + (size_t)bidx * pk_size(N);
        const int t = lane, It = t >> 4;
        const int lbase = (It * (It + 1) / 2) * 256 + wave * 16 + (t & 15);
        double v[16];
        if (!here) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = 4 * u + wave;
                const bool in = j < N && t >= j && t < N;
                v[u] = gL[in ? pkcol(N, j) + t : 0];
            }
        }
        const double mu0 = (tid < Nq) ? gmean[tid] : 0.0;
        const int t0 = (tid && tid < NSO3) ? 9 + 6 * tid : 3;
        const double pdg = gP[t0 * (N + 1)] + gP[(t0 + 1) * (N + 1)] + gP[(t0 + 2) * (N + 1)];
        const double tabv = fast_series_table[tid < 26 ? tid : 25];
        bad = here ? 0 : (a.wsfail[bidx] >= 0);
        bool ok = true;
        int cps[4], cmax = 0;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double cf = mp[4 * f + 3];
            const bool in = (cf >= 0.0) && (cf <= (double)K);
            ok = ok && in;
            cps[f] = __builtin_amdgcn_readfirstlane(in ? (int)cf : 0);   // (the clamp of h(X): plan and addresses from the same indices)
            cmax = cps[f] > cmax ? cps[f] : cmax;
        }
        jmax = __builtin_amdgcn_readfirstlane((cmax ? 6 + 6 * cmax : 0) + 5);
        ksmax = jmax >> 2;
        // the release plan (slk_math.hpp), the same in every wave: all of them count the same barriers.  The factor through the
        // workspace has nothing to release: the single-release plan of its ksmax (every feature on the newest observed pose)
        // keeps the second-pass rule, its mask is not used
        bool single = !here;
#ifdef SLK_STAMPS
        single = single || a.stop == 3;                         // (a run that leaves at stamp 3: the waves 1 - 3 are gone behind the first release)
#endif
        plan = single ? fast_release_plan(cmax, cmax, cmax, cmax, K, 0, true)
                      : fast_release_plan(cps[0], cps[1], cps[2], cps[3], K, SLK_RELEASE_HC, SLK_RELEASE_NEED_C != 0);
        plan.mask = (unsigned)__builtin_amdgcn_readfirstlane((int)plan.mask);      // (two scalar registers: the mask dies with
        plan.word = (unsigned)__builtin_amdgcn_readfirstlane((int)plan.word);      // wave 0's last step, the word with phase 2)
        bad |= !ok;
        if (tid < NSO3) bad |= !(pdg < 9.869604401089358);
        if (tid < Nq) mu[tid] = mu0;
        if (tid < 64) ints[tid] = 0;                    // (str, pd, d0, md32: behind phase 1 -- the factorisation's colbuf lies on them)
        if (tid < 26) T[tid] = tabv;
        if (!here) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = 4 * u + wave;
                const bool in = j < N && t >= j && t < N;
                if ((u >> 2) < NT && It >= (u >> 2) && It < NT) Lt[lbase + (u >> 2) * 256 + (u & 3) * 64] = in ? v[u] : 0.0;
            }
        }
        // (after the stores above: the sixteen loaded values must not live across this region)
        if (here) {
            // wave 0 issues its loads of P, the other three (idle from here to the barrier of phase 0) zero-fill the tiles, and
            // one barrier puts the fill before wave 0's first tile store: the factorisation then stores a column under the
            // lane mask row >= column alone, and reads its rank-4 fragments back from the tiles (CholPSteps, OUT == 2)
            d4 fa[CholM<NT>::NTL];
            if (wave == 0) cholm_load_t_exact<NT, N>(fa, gP, lane);
            else {
                double2 *Lt2 = reinterpret_cast<double2 *>(Lt);
                for (int e = tid - 64; e < CholM<NT>::NTL * 128; e += NTHREADS - 64) Lt2[e] = double2{0.0, 0.0};   // (every wave but wave 0)
            }
            __syncthreads();
            // RELEASE: h(X) of a feature on pose c reads the rows tp .. tp + 5 of the factor at the columns j <= tp + 5 <= jmax,
            // and step s of the factorisation leaves L(t, j) final for every j <= 4 s + 3.  Behind the tile stores of every step
            // in plan.mask (fast_release_plan, slk_math.hpp: every bit a live step 0 .. NKS - 1, because cp <= K, so each barrier
            // is always met) wave 0 meets the other three in a workgroup barrier and runs its remaining steps -- columns which
            // nothing reads before the next release or the barrier that closes phase 1 -- while they work on what is final:
            //   one bit, ksmax (the step that holds column jmax): every feature behind it; with the newest pose observed
            //     (ksmax = NKS - 1) the barrier stands at the end of the factorisation;
            //   staggered, A < B = ksmax [< C]: the two features that are final first behind A, the other two behind B, S and
            //     the prefix sums (which read only what h(X) wrote) behind C.
            // The other waves count their barriers from the plan's flags (phase 1), wave 0 from the mask: the same number.
            // colbuf = [oRef, oStr + 64): ref, delta, md32, d0, d0s, pd, cq, str -- all first written behind phase 1.  The union
            // region, where it used to be, holds what the released waves write while wave 0 factors on: Yp, dZ, innov, dz0 of
            // the early h(X), tmpS and Sm of an early S.  The factorisation never touches that region.
            static_assert(CholM<NT>::COLBUF <= F::oStr + 64 - F::oRef, "colbuf fits the arrays of the gain phase and the mean loop");
            if (wave == 0) {
#ifdef SLK_STAMPS
                int nrel = 0;                                   // (stamps: wave 0 reaches / leaves the barriers A, B, C at 1 / 2, 9 / 10, 5 / 31)
#endif
                bad |= cholp_factor<NT, 2, N>(fa, Lt, N, ref, lane, plan.mask, [&]() __attribute__((always_inline)) {
                    wave_sync();                                // (the tile stores of this step and every one before it)
#ifdef SLK_STAMPS
                    SLK_WSTAMP(0, nrel == 0 ? 1 : (nrel == 1 ? 9 : 5));
#endif
                    __builtin_amdgcn_s_barrier();
#ifdef SLK_STAMPS
                    SLK_WSTAMP(0, nrel == 0 ? 2 : (nrel == 1 ? 10 : 31));
                    ++nrel;
#endif
                }) >= 0;
            } else {
                __syncthreads();                                // (the first release: A, or the only one)
            }
        } else {
            __syncthreads();                                    // (the factor through the workspace: every wave stored its part of the tiles)
        }
    }
    SLK_FSTAMP(3);                                              // (thread 0: the end of the factorisation)

    // ---- phase 1: Z = h(X) (Msckf.hpp:231-232), one wave per feature and pass, lane j = the sigma pair of column j.  Waves
    // 1 - 3 start behind the first release above, wave 0 behind its last step; the filter may be one that is about to leave
    // (failed factorisation, bad pose index, rotation bound -- decided in the barrier that closes this phase): the pose index
    // is clamped before it forms an address, everything else h(X) reads lies at addresses that do not depend on data.
    // Which wave takes which feature in which pass is the plan's (fast_release_plan): the body writes Yp, dZ, innov and dz0 by
    // FEATURE index, so the assignment changes no bit.  ONE copy of the code, a uniform loop over the two passes.
    //   single release: every wave its own feature.  Feature 0: with R = wave 0's steps behind the release and H = one h(X),
    //     wave 0 taking it ends the phase at R + H, wave 1 taking it as a second pass at max(R, 2 H) -- ahead when R >= H.  H is
    //     about the time of three of the late steps (profiles/README.md), so the second pass runs when at least three steps
    //     follow the release;
    //   staggered: the waves 1 and 2 take the two features that are final first behind A and, behind one more barrier that
    //     every wave but wave 0 meets here (wave 0: in its step B), the other two.  Wave 0 takes none.  A released wave that is
    //     late makes wave 0 wait in its next release; nothing but time depends on the estimate H.
    const bool staggered = fast_plan_staggered(plan);
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && staggered && wave != 0) __syncthreads();  // B
        const int f = fast_plan_feature(plan, wave, pass);
        if (f == FAST_PLAN_NONE) continue;
        if (pass == 0) { SLK_WSTAMP(0, 17); SLK_WSTAMP(1, 19); }
        const double cf = mp[4 * f + 3];
        const int cp = (cf >= 0.0 && cf <= (double)K) ? (int)cf : 0;
        const int tp = cp ? 6 + 6 * cp : 0, sp = cp ? 6 + 7 * cp : 0;
        const double fx = mp[4 * f], fy = mp[4 * f + 1], fz = mp[4 * f + 2];
        const int j = lane, Jc = j >> 4;
        const bool act = j < tp + 6;                            // column j reaches the pose's six rows
        double l[6], x[7];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int t = tp + q, I = t >> 4;
            const bool in = act && Jc <= I;
            l[q] = Lt[in ? (I * (I + 1) / 2 + Jc) * 256 + (j & 15) * 16 + (t & 15) : 16];     // Lt[16] = L(0, 1) = 0
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) x[q] = mu[sp + q];
        double zp0, zp1, zm0, zm1;
        {
            const double rv[2][3] = {{l[3], l[4], l[5]}, {-l[3], -l[4], -l[5]}};
            Quat ex[2];
            so3_exp_tab_flag<2>(T, rv, ex, ints + 50);               // (set by a rotation column beyond the series' domain, 4 rad)
            const Quat qx = Quat{x[3], x[4], x[5], x[6]};
            double lx, ly, lz;
            // (x / z by one refined reciprocal and a correction step: within an ulp of the IEEE quotient, half the instructions
            // of two divisions)
            auto quot = [](double lx_, double ly_, double lz_, double &q0, double &q1) __attribute__((always_inline)) {
                const double r = rcp_refined(lz_);
                q0 = lx_ * r; q0 = fma(fma(-lz_, q0, lx_), r, q0);
                q1 = ly_ * r; q1 = fma(fma(-lz_, q1, ly_), r, q1);
            };
            qrot(qconj(qmul_exp(qx, ex[0])), fx - (x[0] + l[0]), fy - (x[1] + l[1]), fz - (x[2] + l[2]), lx, ly, lz);
            quot(lx, ly, lz, zp0, zp1);
            qrot(qconj(qmul_exp(qx, ex[1])), fx - (x[0] - l[0]), fy - (x[1] - l[1]), fz - (x[2] - l[2]), lx, ly, lz);
            quot(lx, ly, lz, zm0, zm1);
        }
        const double Z00 = readlane_f64(zp0, 63), Z01 = readlane_f64(zp1, 63);       // lanes >= tp + 6 evaluate X_0
        const double yp0 = zp0 - Z00, yp1 = zp1 - Z01, ym0 = zm0 - Z00, ym1 = zm1 - Z01;
        Yp[j * 17 + 2 * f] = yp0; Yp[j * 17 + 2 * f + 1] = yp1;
        Yp[j * 17 + 8 + 2 * f] = ym0; Yp[j * 17 + 8 + 2 * f + 1] = ym1;
        dZi[f * 128 + 2 * j] = yp0 - ym0; dZi[f * 128 + 2 * j + 1] = yp1 - ym1;
        const double s0 = wave_sum_f64(yp0 + ym0), s1 = wave_sum_f64(yp1 + ym1);
        if (lane == 0) {                                        // mean_z (:234) about Z_0, innovation (:236)
            const double e0 = s0 * (1.0 / (double)S), e1 = s1 * (1.0 / (double)S);
            innov[2 * f] = a.z[(size_t)bidx * 8 + 2 * f] - (Z00 + e0);
            innov[2 * f + 1] = a.z[(size_t)bidx * 8 + 2 * f + 1] - (Z01 + e1);
            dz0[2 * f] = e0; dz0[2 * f + 1] = e1;
        }
        SLK_WSTAMP(0, 18); SLK_WSTAMP(1, 21);
    }
    // ---- phase 2: S = 1/2 sum (Z_i - mean_z)(Z_i - mean_z)^T + R (:238) on wave 1, the prefix sums of the factor update on
    // wave 3: ONE copy of the code, with the barrier that closes phase 1 in front of it or behind it.  Both read only what h(X)
    // wrote (Yp, dZ, dz0; R from memory), at addresses that do not depend on data, and write registers (wave 3) and tmpS / Sm in
    // the union region, which the factorisation never touches.  So
    //   with a release C in the plan (early_s) they run behind C, under wave 0's last steps and possibly on a filter that is
    //     about to leave; the closing barrier follows and is also the barrier behind S -- it separates wave 1's reads of Yp
    //     from wave 3's fast_prefix_park below;
    //   without one the closing barrier comes first and S has a barrier of its own behind it, as before.
    // (S in two places instead, each writing Gs / Gt: 128 VGPRs and 368 B of scratch at k = 8 -- the sums meet in fifty phis.)
    // The barrier that closes phase 1 is the one in which the conditions of phase 0 meet: failed factorisation, bad index and
    // rotation bound first, then the flag of h(X)'s exponential -- every bail-out before any global write, whatever ran early.
    // The zeros of str / pd / d0 / md32 stay behind it: wave 0's colbuf lies on them until its last step.
    // Gs and Gt live across the closing barrier when S is early (else across the barrier behind S, as before), and the park.
    double Gs[NKS - 1], Gt[36];                                 // wave 3: the factor update's prefix sums, block bases and tails
    const bool early_s = fast_plan_has_c(plan);
    // (the closing barrier with its bail-outs and zeros: two copies of a barrier and four stores, ONE of S and the prefix sums)
    auto close_phase1 = [&]() __attribute__((always_inline)) {
        if (__syncthreads_or(bad)) return 2;
        if (ints[50]) return 3;
        // (the factorisation's colbuf is dead: the zeros these arrays start from; their first readers are phases away)
        if (tid < 64) { str[tid] = 0.0; pd[tid] = 0.0; }
        if (tid < 32) { d0[tid] = 0.0; md32[tid] = 0.0; }
        return 0;
    };
    if (!early_s) {
        if (const int code = close_phase1()) SLK_FBAIL(code);
        SLK_FSTAMP(4);
    } else if (wave != 0) {
        __syncthreads();                                        // C
    }
    if (wave == 1) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        fast_steps_to<0, NKS>(ksmax, [&](auto ix) __attribute__((always_inline)) {      // (the columns beyond jmax hold y+ = y- = 0)
            constexpr int ks = decltype(ix)::value;
            const double fr = Yp[ks * 68 + g4 * 17 + c16];      // rows [y+ ; y-] of column 4 ks + g
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fr, fr, acc, 0, 0, 0);
        });
        if (c16 < 8) { tmpS[g4 + 8 * c16] = acc[0]; tmpS[g4 + 4 + 8 * c16] = acc[1]; }
        else { tmpS[64 + g4 + 8 * (c16 - 8)] = acc[2]; tmpS[64 + g4 + 4 + 8 * (c16 - 8)] = acc[3]; }
        wave_sync();
        const double *R = a.R + (size_t)bidx * a.r_stride;
        const int row = lane & 7, col = lane >> 3;
        Sm[lane] = 0.5 * ((tmpS[lane] + tmpS[64 + lane]) - (double)S * dz0[row] * dz0[col]) + R[lane];
        SLK_WSTAMP(1, 16);
    } else if (wave == 3) {
        // prefix sums over the columns of dZ dZ^T for the factor update (fast_prefix_blocks): the base of every block of four
        // columns from an MFMA chain beside S's, kept in registers -- no LDS is free before S is done.  On the wave that
        // consumes them: its hand-over through LDS below needs no barrier.
        fast_prefix_tail(dZi, lane, Gt);                        // each column's sum inside its block
        __builtin_amdgcn_sched_barrier(0);                      // (tails, then the chain: the neighbours' deviations are dead by then)
        fast_prefix_blocks<NKS>(dZi, c16, g4, Gs);              // (no stamp here: with one the stamps build spills 42 registers)
    }
    if (early_s) {
        if (const int code = close_phase1()) SLK_FBAIL(code);
        SLK_FSTAMP(4);
    } else {
        __syncthreads();
    }
    SLK_FSTAMP(6);
    // The block bases go to the Yp rows (dead: S is done), the first min(ksmax + 2, NKS) slots of [0, NKS * kPrefixSlot) of the
    // union (the slots behind them are neither written nor read), from the MFMA layout to lane = column: wave 3 alone writes
    // and reads them, no barrier.  Ahead of the gate: their registers are free across it.  Wb aliases [0, 512): every base is
    // read before fast_ldm_columns' first Wb store (the stores are its last step, behind the last column of T).
    if (wave == 3) {
        fast_prefix_park<NKS>(Yp, c16, g4, ksmax, Gs);
        wave_sync();
    }

    // ---- gate: removeOutliers (:723-754) with the shifted second erase (:741-744); every wave takes the same decisions
    unsigned kept = 0xffu, nout = 0u;
    if (a.gate) {
        const int p = 2 * (lane & 3), q = p + 1;
        const double s00 = Sm[p + 8 * p], s01 = Sm[p + 8 * q], s10 = Sm[q + 8 * p], s11 = Sm[q + 8 * q];
        const double det = s00 * s11 - s01 * s10, r0 = innov[p], r1 = innov[q];
        const double d2 = (r0 * (s11 * r0 - s01 * r1) + r1 * (s00 * r1 - s10 * r0)) / det;
        if (!__all(d2 < 5.99)) {                                // chi2_0.95(2), Msckf.hpp:861-865
            int *ix = ints + 10 * wave;
            if (lane == 0) {
                int cnt = 8, i = 0;
                unsigned no = 0;
                for (int r = 0; r < 8; ++r) ix[r] = r;
                while (i < cnt / 2) {
                    const int pp = ix[2 * i], qq = ix[2 * i + 1];
                    const double t00 = Sm[pp + 8 * pp], t01 = Sm[pp + 8 * qq], t10 = Sm[qq + 8 * pp], t11 = Sm[qq + 8 * qq];
                    const double dt = t00 * t11 - t01 * t10, u0 = innov[pp], u1 = innov[qq];
                    const double dd = (u0 * (t11 * u0 - t01 * u1) + u1 * (t00 * u1 - t10 * u0)) / dt;
                    if (!(dd < 5.99)) {
                        for (int rep = 0; rep < 2; ++rep) {     // removeRow semantics, :688-697
                            const int pos = 2 * i + rep, numRows = cnt - 1;
                            if (pos < numRows) for (int w = pos; w < numRows; ++w) ix[w] = ix[w + 1];
                            cnt = numRows;
                        }
                        no++;
                    } else {
                        i++;
                    }
                }
                unsigned kp = 0;
                for (int r = 0; r < cnt; ++r) kp |= 1u << ix[r];
                ix[8] = (int)kp; ix[9] = (int)no;
            }
            wave_sync();
            kept = (unsigned)ix[8]; nout = (unsigned)ix[9];
        }
    }
    if (kept == 0u) SLK_FBAIL(4);                               // every block rejected (:250): status by the general body
    SLK_FSTAMP(7);

    // ---- gain side.  wave 3: columns of the factor update.  wave 0: x = S^-1 nu over the surviving rows (rejected rows
    // as identity rows), b = 1/2 dZ x, delta = K nu = L b (:257, :263), then the reference point of the mean loop.
    if (wave == 0) {
        double gg[8][8], gi[8], y[8];
        // (set-up with every row kept -- kept is wave-uniform and nearly always 0xff -- without the selects; one chain for both.
        // The innovation keeps its select inside the chain: held here it is eight more doubles live beside the 36 entries)
        if (kept == 0xffu) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) gg[i][j] = Sm[i + 8 * j];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    const bool in = ((kept >> i) & 1u) && ((kept >> j) & 1u);
                    const double v = Sm[in ? i + 8 * j : 0];
                    gg[i][j] = in ? v : (i == j ? 1.0 : 0.0);
                }
            }
        }
        bool spd = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            double d = gg[j][j];
#pragma unroll
            for (int p = 0; p < j; ++p) d = fma(-gg[j][p], gg[j][p], d);
            spd = spd && (d > 0.0);
            double sq, rs;
            rsqrt_pivot(d, sq, rs);
            gi[j] = rs;
#pragma unroll
            for (int i = j + 1; i < 8; ++i) {
                double v = gg[i][j];
#pragma unroll
                for (int p = 0; p < j; ++p) v = fma(-gg[i][p], gg[j][p], v);
                gg[i][j] = v * rs;
            }
            double s = ((kept >> j) & 1u) ? innov[j] : 0.0;
#pragma unroll
            for (int p = 0; p < j; ++p) s = fma(-gg[j][p], y[p], s);
            y[j] = s * rs;
        }
#pragma unroll
        for (int cc = 7; cc >= 0; --cc) {
            double s = y[cc];
#pragma unroll
            for (int p = cc + 1; p < 8; ++p) s = fma(-gg[p][cc], y[p], s);
            y[cc] = s * gi[cc];
        }
        if (!spd && lane == 0) ints[49] = 1;
        SLK_WSTAMP(0, 24);
        double bj = 0.0;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) bj = fma(dZi[(cc >> 1) * 128 + 2 * lane + (cc & 1)], y[cc], bj);
        bvec[lane] = 0.5 * bj;                                   // rows >= N of dZ are zero
        wave_sync();
        {
            const int t = lane, It = t >> 4;
            const double *Lrow = Lt + (It * (It + 1) / 2) * 256 + (t & 15);
            double part[NT];
#pragma unroll
            for (int Jb = 0; Jb < NT; ++Jb) part[Jb] = 0.0;
            // groups of eight columns up to the one that holds jmax: b_j = 0 beyond it, the sums stay what they are
            fast_steps_to<0, 2 * NT>(jmax >> 3, [&](auto ix) __attribute__((always_inline)) {
                constexpr int Jb = decltype(ix)::value >> 1, j0 = 8 * (decltype(ix)::value & 1);
                double s = part[Jb];
#pragma unroll
                for (int jj = j0; jj < j0 + 8; ++jj)
                    if (16 * Jb + jj < N) s = fma(Lrow[Jb * 256 + jj * 16], bvec[16 * Jb + jj], s);
                part[Jb] = s;
                __builtin_amdgcn_sched_barrier(0);               // (eight columns of loads in flight at a time: registers)
            });
            double dl = part[0];
#pragma unroll
            for (int Jb = 1; Jb < NT; ++Jb) dl += (It >= Jb) ? part[Jb] : 0.0;      // (tile columns right of the row's own hold other tiles)
            if (t < 64) delta[t] = (t < N) ? dl : 0.0;
            const int s = (t < N) ? fast_vec_storage(t) : -1;
            if (s >= 0) ref[s] = mu[s] + dl;                     // X_0 = mu [+] delta (:501), vector part
        }
        wave_sync();
        if (lane < NSO3) {
            const int to = lane ? 9 + 6 * lane : 3, so = lane ? 9 + 7 * lane : 3;
            const Quat qm = ldq(mu + so);
            const double dv[1][3] = {{delta[to], delta[to + 1], delta[to + 2]}};
            Quat ex[1];
            so3_exp_tab_flag<1>(T, dv, ex, ints + 50);
            const Quat qr = qmul_exp(qm, ex[0]);
            stq(ref + so, qr);
            stq(cq + 4 * lane, qmul(qconj(qr), qm));
        }
        SLK_WSTAMP(0, 25);
    }
    else if (wave == 3) {
        SLK_WSTAMP(3, 22);
        const double *bp = Yp + fast_prefix_slot(lane, ksmax, NKS) * kPrefixSlot;       // (dead lanes: the last live block)
        const bool pdok = fast_ldm_columns(Gt, bp, dZi, Sm, kept, lane, N, Wb, mdiag);
        if (!pdok && lane == 0) ints[48] = 1;
        SLK_WSTAMP(3, 23);
    }
    __syncthreads();
    if (ints[48] | ints[49] | ints[50]) SLK_FBAIL(5);                      // indefinite downdate / non-SPD S / large rotation: the general body decides
    SLK_FSTAMP(8);

    // ---- applyDelta's factor: L' = L chol(I - B B^T) (:262-263, :659-662)
    unsigned long long pt0 = 0, pt1 = 0;                       // pair descriptors of the mean loop
    ldm_product_tiled<NT>(Lt, dZi, Wb, mdiag, lane, wave, jmax, [&]() {
        pt0 = FastPairTableHolder<K>::tab.v[tid < NP ? tid : 0];
        pt1 = FastPairTableHolder<K>::tab.v[(wave == 1 && 256 + lane < NP) ? 256 + lane : 0];
        for (int e = tid; e < NKS * 128; e += 256) Et[e] = 0.0;
    });
    SLK_FSTAMP(11);

    // ---- manifold mean of the re-drawn sigma points (:664 -> :499-525) over (block, column) pairs: round 0 on every wave,
    // the pairs beyond 256 on wave 1, the centre points (one deviation each) on wave 2, the row sums on waves 2 / 3
    constexpr int RP = (NP + 255) / 256;                         // rounds of pairs (2 for k >= 7)
    int aL[RP][3], aE0[RP], bsd[RP];                            // (component 1 / 2 of E^ and the row-15 case are derived at use)
    bool val[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) {
        const unsigned long long w = r ? pt1 : pt0;
        const unsigned lo = (unsigned)w, hi = (unsigned)(w >> 32);
        val[r] = (r ? 256 + lane : tid) < NP && (r == 0 || wave == 1);
        bsd[r] = lo >> 26;                                       // block | odd-part-to-str case << 4
        aL[r][0] = lo & 0x1fff; aL[r][1] = (lo >> 13) & 0x1fff; aL[r][2] = hi & 0x1fff;
        aE0[r] = (hi >> 13) & 0x7ff;
    }
    auto e_off = [](int e0, int b, int cc) __attribute__((always_inline)) {     // offset of component cc in E^
        const int rho = 3 * b;                                   // (a component that crosses into the second 16 rows: + 49)
        const int e1 = e0 + ((rho & 15) == 15 ? 49 : 1);
        return cc == 0 ? e0 : (cc == 1 ? e1 : e1 + (((rho + 1) & 15) == 15 ? 49 : 1));
    };
    double dpl[RP][3], dmi[RP][3], dc[3] = {0.0, 0.0, 0.0};
    int it = 0;
    for (;;) {
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            if (r == 0 ? 64 * wave >= NP : wave != 1) continue;  // nothing for this wave in this round
            const int b = bsd[r] & 15, to = b ? 9 + 6 * b : 3;
            const double l0 = smem[aL[r][0]], l1 = smem[aL[r][1]], l2 = smem[aL[r][2]];
            const double e0 = delta[to], e1 = delta[to + 1], e2 = delta[to + 2];
            const Quat cb = ldq(cq + 4 * b);
            const double rv[2][3] = {{e0 + l0, e1 + l1, e2 + l2}, {e0 - l0, e1 - l1, e2 - l2}};
            Quat ex[2];
            double dd[2][3];
            so3_exp_tab_flag<2>(T, rv, ex, ints + 50);          // (set beyond the series' domain; the log has none)
            ex[0] = qmul_exp(cb, ex[0]);
            ex[1] = qmul_exp(cb, ex[1]);
#ifdef SLK_STAMPS
            {   // diagnostic: which waves leave the direct series (bit 0 / 1 of round r: exp / log went the angle-halving way)
                bool se = true, sl = true;
                for (int i = 0; i < 2; ++i) {
                    se = se && (0.25 * (rv[i][0] * rv[i][0] + rv[i][1] * rv[i][1] + rv[i][2] * rv[i][2]) < 0.25);
                    const double n2 = ex[i].x * ex[i].x + ex[i].y * ex[i].y + ex[i].z * ex[i].z;
                    sl = sl && (ex[i].w > 0.0) && (n2 * 16.0 < ex[i].w * ex[i].w);
                }
                const int code = (__all(se) ? 0 : 1) | (__all(sl) ? 0 : 2);
                const int slot = wave < 2 ? 26 + wave : 27 + wave;
                if (lane == 0 && a.dbg && it == 0) a.dbg[(size_t)bidx * 32 + slot] = (r ? a.dbg[(size_t)bidx * 32 + slot] : 0) | (code << (2 * r));
            }
#endif
            so3_log_tab<2>(T, ex, dd);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) { dpl[r][cc] = dd[0][cc]; dmi[r][cc] = dd[1][cc]; }
            if (val[r]) {
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) Et[e_off(aE0[r], b, cc)] = 0.5 * (dpl[r][cc] + dmi[r][cc]);
            }
        }
        if (wave == 2) {                                         // X_0 [-] ref per block
            const int b = lane < NSO3 ? lane : 0, to = b ? 9 + 6 * b : 3;
            const double rv[1][3] = {{delta[to], delta[to + 1], delta[to + 2]}};
            const Quat cb = ldq(cq + 4 * b);
            Quat ex[1];
            double dd[1][3];
            so3_exp_tab_flag<1>(T, rv, ex, ints + 50);
            ex[0] = qmul_exp(cb, ex[0]);
            so3_log_tab<1>(T, ex, dd);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                dc[cc] = dd[0][cc];
                if (lane < NSO3) {                               // (the points beyond the block's columns: weight S - 2 (toff + 3))
                    d0[3 * b + cc] = dc[cc];
                    d0s[3 * b + cc] = (double)(S - 2 * (b ? 12 + 6 * b : 6)) * dc[cc];
                }
            }
        }
        __syncthreads();
        if (ints[50]) SLK_FBAIL(6);                              // (nothing has been written yet: the general body starts over)
        // mean_delta = sum_i (X_i [-] ref) / S (:507-509): the S - 2 (toff + 3) points beyond the block's columns equal X_0
        if (wave >= 2) {
            const int hr = wave - 2;
            double s = 0.0;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) s += Et[(ks * 2 + hr) * 64 + lane];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            const int rho = 16 * hr + lane;                      // (lanes 0 .. 15 hold the sums of the rows 16 hr ..)
            // |mean_delta|^2 where mean_delta is formed: each row of sixteen lanes sums its squares (four row shifts, lane 15
            // ends with the row's sum; a wave without live rows -- wave 3 at k = 4 -- sums zeros), one partial sum per wave
            double sq = 0.0;
            if (lane < 16 && rho < NROT) {
                const double mv = (2.0 * s + d0s[rho]) * (1.0 / (double)S);
                md32[rho] = mv;
                sq = mv * mv;
            }
            sq += dpp_mov_f64<0x111, 0xf>(sq);                   // row_shr:1
            sq += dpp_mov_f64<0x112, 0xf>(sq);                   // row_shr:2
            sq += dpp_mov_f64<0x114, 0xf>(sq);                   // row_shr:4
            sq += dpp_mov_f64<0x118, 0xf>(sq);                   // row_shr:8
            if (lane == 15) msq[hr] = sq;
        }
        __syncthreads();
        // every lane of every wave reads the same two doubles and adds them in the same order: one decision from the same
        // bits, taken as a ballot (wave-uniform by construction; all lanes agree, so it is none or all of them)
        const bool more = __builtin_amdgcn_ballot_w64(msq[0] + msq[1] > MEAN_STOP_SQ) != 0ull;   // :511, |mean_delta| > 1e-6 on the squared norm (slk_math.hpp)
        if (wave == 0 && lane < NSO3) {                          // reference += mean_delta (:510)
            const int so = lane ? 9 + 7 * lane : 3;
            const double dv[1][3] = {{md32[3 * lane], md32[3 * lane + 1], md32[3 * lane + 2]}};
            Quat ex[1];
            so3_exp_tab_flag<1>(T, dv, ex, ints + 50);           // (a mean_delta beyond 4 rad)
            const Quat qr = qmul_exp(ldq(ref + so), ex[0]);
            stq(ref + so, qr);
            stq(cq + 4 * lane, qmul(qconj(qr), ldq(mu + so)));
        }
        if (!more) break;
        if (++it >= 64) SLK_FBAIL(7);                            // (nothing has been written yet: the general body starts over)
        __syncthreads();
    }
    SLK_FSTAMP(12);
    SLK_NOTE(20, it + 1);
    // The loop leaves with |mean_delta| <= 1e-6: deviations against the FINAL mean by the first-order correction
    //     d' = d - Jl^-1(d) m,  Jl^-1(d) m = m - 1/2 d x m + (1/12 + |d|^2 / 720) d x (d x m)       (slk_kernels.hpp)
    // then the odd parts into the rotation rows of the factor array, the even parts minus the centre into E^.
    {
        auto fix = [&](double &x, double &y, double &z, double m0, double m1, double m2) __attribute__((always_inline)) {
            const double cx = y * m2 - z * m1, cy = z * m0 - x * m2, cz = x * m1 - y * m0;      // d x m
            const double ax = y * cz - z * cy, ay = z * cx - x * cz, az = x * cy - y * cx;      // d x (d x m)
            const double a12 = 1.0 / 12.0 + (x * x + y * y + z * z) * (1.0 / 720.0);
            x = x - m0 + 0.5 * cx - a12 * ax;
            y = y - m1 + 0.5 * cy - a12 * ay;
            z = z - m2 + 0.5 * cz - a12 * az;
        };
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            if (r == 0 ? 64 * wave >= NP : wave != 1) continue;
            const int b = bsd[r] & 15, sd = bsd[r] >> 4;
            const double m0 = md32[3 * b], m1 = md32[3 * b + 1], m2 = md32[3 * b + 2];
            double c0 = d0[3 * b], c1 = d0[3 * b + 1], c2 = d0[3 * b + 2];
            fix(c0, c1, c2, m0, m1, m2);
            fix(dpl[r][0], dpl[r][1], dpl[r][2], m0, m1, m2);
            fix(dmi[r][0], dmi[r][1], dmi[r][2], m0, m1, m2);
            if (val[r]) {
                smem[sd ? F::oStr + 16 * sd - 1 : aL[r][0]] = 0.5 * (dpl[r][0] - dmi[r][0]);    // (row 15's columns 16 / 17: str)
                smem[aL[r][1]] = 0.5 * (dpl[r][1] - dmi[r][1]);
                smem[aL[r][2]] = 0.5 * (dpl[r][2] - dmi[r][2]);
                Et[e_off(aE0[r], b, 0)] = 0.5 * (dpl[r][0] + dmi[r][0]) - c0;
                Et[e_off(aE0[r], b, 1)] = 0.5 * (dpl[r][1] + dmi[r][1]) - c1;
                Et[e_off(aE0[r], b, 2)] = 0.5 * (dpl[r][2] + dmi[r][2]) - c2;
            }
        }
        if (wave == 2 && lane < NSO3) {
            fix(dc[0], dc[1], dc[2], md32[3 * lane], md32[3 * lane + 1], md32[3 * lane + 2]);
            pd[32 + 3 * lane] = dc[0]; pd[32 + 3 * lane + 1] = dc[1]; pd[32 + 3 * lane + 2] = dc[2];
        }
    }
    __syncthreads();
    if (ints[50]) SLK_FBAIL(8);                                  // (the last move of the reference was beyond 1 rad)
    // the new mean (:664): no fallback beyond this point
    double *omean = a.mean_out ? a.mean_out + (size_t)bidx * Nq : a.mean + (size_t)bidx * Nq;
    double *oP = a.P_out ? a.P_out + (size_t)bidx * N * N : a.P + (size_t)bidx * N * N;
    if (wave == 1 && lane < N) {
        const int sv = fast_vec_storage(lane);
        if (sv >= 0) omean[sv] = ref[sv];
    }
    if (wave == 0 && lane < NSO3) {
        const int so = lane ? 9 + 7 * lane : 3;
        const Quat qr = ldq(ref + so);
        omean[so] = qr.x; omean[so + 1] = qr.y; omean[so + 2] = qr.z; omean[so + 3] = qr.w;
    }
    if (tid == 0) a.outliers[bidx] = nout;
    SLK_FSTAMP(13);

    // ---- P+ (:665 -> :574-589): p = sum_j e^_j + (N + 1/2) / 2 d0 by waves 2 / 3, the tile columns one per wave
    if (wave >= 2) {
        const int hr = wave - 2;
        double s = 0.0;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) s += Et[(ks * 2 + hr) * 64 + lane];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        const int rho = 16 * hr + lane;
        if (lane < 16 && rho < NROT) pd[rho] = s + (0.5 * ((double)N + 0.5)) * pd[32 + rho];
    }
    // E^ E^^T where E^ lives: tile (0, 0) on wave 0, (1, 0) on wave 2, (1, 1) on wave 3; published over E^ once every wave
    // has read its fragments and row sums
    using EE = FastEE<K>;
    static_assert(NROT <= EE::PAD && EE::wave_of(0, 0) == 0 && EE::wave_of(1, 0) == 2 && EE::wave_of(1, 1) == 3, "EE tiles");
    d4 eacc = {0.0, 0.0, 0.0, 0.0};
    if (wave == 0) eacc = fast_ee_tile<K, 0, 0>(Et, lane);
    else if constexpr (EE::NTE > 1) {
        if (wave == 2) eacc = fast_ee_tile<K, 1, 0>(Et, lane);
        else if (wave == 3) eacc = fast_ee_tile<K, 1, 1>(Et, lane);
    }
    __syncthreads();                                             // E^ is dead; p and the corrected d0 are complete
    double *ee = U;
    if (wave == 0) fast_ee_publish<K, 0, 0>(ee, lane, fast_ee_rank2<0, 0>(pd, lane, eacc));
    else if constexpr (EE::NTE > 1) {
        if (wave == 2) fast_ee_publish<K, 1, 0>(ee, lane, fast_ee_rank2<1, 0>(pd, lane, eacc));
        else if (wave == 3) fast_ee_publish<K, 1, 1>(ee, lane, fast_ee_rank2<1, 1>(pd, lane, eacc));
    }
    d4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    if (wave == 0) fast_rebuild_col<K, 0>(Lt, str, lane, acc);
    else if (wave == 1) fast_rebuild_col<K, 1>(Lt, str, lane, acc);
    else if (wave == 2) fast_rebuild_col<K, 2>(Lt, str, lane, acc);
    else if constexpr (NT > 3) fast_rebuild_col<K, 3>(Lt, str, lane, acc);
    __syncthreads();                                             // the factor is dead; EE is complete
    SLK_FSTAMP(14);
    if (wave == 0) fast_store_col<K, 0>(ee, Lt, oP, lane, acc, a.lower_only != 0);
    else if (wave == 1) fast_store_col<K, 1>(ee, Lt, oP, lane, acc, a.lower_only != 0);
    else if (wave == 2) fast_store_col<K, 2>(ee, Lt, oP, lane, acc, a.lower_only != 0);
    else if constexpr (NT > 3) fast_store_col<K, 3>(ee, Lt, oP, lane, acc, a.lower_only != 0);
    SLK_STAMP_NR(15);
    return true;
}

} // namespace slk
