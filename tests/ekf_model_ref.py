"""Reference linearisation of SLK_MM_FEATURE_PROJ for the EKF-from-model tests: a small analytic numpy Jacobian (checked
against central differences of the oracle's own model and boxplus by the CPU suite), the oracle's h, and the inputs the
tests share.  No product.  quat_matrix, skew and linearize_np are pure numpy; the functions that need the oracle import
it themselves, so that a tool can borrow the numpy Jacobian without the oracle being built."""
import ctypes as C

import numpy as np

import scenarios as sc

CHI2 = 5.99                                   # the gate's threshold, chi2_0.95(2) (Msckf.hpp:861-865)
SHAPES = [(8, 128), (8, 60), (4, 64), (9, 80), (0, 12), (31, 512)]       # (k, m)


def quat_matrix(q):
    """Rotation matrices [..., 3, 3] of quaternions [..., 4] stored (x, y, z, w)."""
    x, y, z, w = np.moveaxis(np.asarray(q, dtype=np.float64), -1, 0)
    R = np.empty(x.shape + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - z * w)
    R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w)
    R[..., 2, 1] = 2 * (y * z + x * w)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def linearize_np(mean, feat, k):
    """mean [B, Nq], feat [B, nf, 4] (landmark xyz, pose index) -> zmean [B, 2 nf], H [B, 2 nf, N] under the filter's
    boxplus (p + dp, q * exp(dtheta)): H_p = -J R^T, H_theta = J [l]x with l = R^T (Lw - p)."""
    mean, feat = np.asarray(mean, dtype=np.float64), np.asarray(feat, dtype=np.float64)
    B, nf = feat.shape[:2]
    N = 12 + 6 * k
    c = feat[..., 3].astype(int)
    sp = np.where(c == 0, 0, 13 + 7 * (c - 1))
    tp = np.where(c == 0, 0, 12 + 6 * (c - 1))
    bi = np.arange(B)[:, None]
    p = np.stack([mean[bi, sp + i] for i in range(3)], axis=-1)
    q = np.stack([mean[bi, sp + 3 + i] for i in range(4)], axis=-1)
    Rt = np.swapaxes(quat_matrix(q), -1, -2)
    l = np.einsum("bfij,bfj->bfi", Rt, feat[..., :3] - p)
    zmean = (l[..., :2] / l[..., 2:3]).reshape(B, 2 * nf)
    J = np.zeros((B, nf, 2, 3))
    J[..., 0, 0] = J[..., 1, 1] = 1.0 / l[..., 2]
    J[..., 0, 2] = -l[..., 0] / l[..., 2] ** 2
    J[..., 1, 2] = -l[..., 1] / l[..., 2] ** 2
    blk = np.concatenate([-J @ Rt, J @ skew(l)], axis=-1)             # [B, nf, 2, 6]
    H = np.zeros((B, 2 * nf, N))
    cols = np.arange(6)[None, :]
    for j in range(nf):
        for r in range(2):
            H[bi, 2 * j + r, tp[:, j, None] + cols] = blk[:, j, r, :]
    return zmean, H


def h_oracle(k, feat_b, x):
    """oracle.mm_feature_proj of one filter's features at the full state x [Nq]."""
    from oracle import oracle as o
    lay = o.layout(o.MULTI, k)
    mod = o.mm_feature_proj(np.ascontiguousarray(feat_b, dtype=np.float64).ravel())
    m = 2 * (np.asarray(feat_b).size // 4)
    z = np.zeros(m)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    o.MEASURE_FN(mod.fn.value)(C.byref(lay), xx.ctypes.data_as(dp), m, z.ctypes.data_as(dp), mod.ctx)
    return z


def central_differences(k, feat_b, x, step=1e-6):
    """dh/d(tangent) of the oracle's model composed with the oracle's boxplus at x, one filter -> [m, N]."""
    from oracle import oracle as o
    lay = o.layout(o.MULTI, k)
    N = 12 + 6 * k
    cols = []
    for t in range(N):
        v = np.zeros(N)
        v[t] = step
        cols.append((h_oracle(k, feat_b, o.boxplus(lay, x, v)) - h_oracle(k, feat_b, o.boxplus(lay, x, -v))) / (2 * step))
    return np.stack(cols, axis=1)


def scenario(k, m, B=4, seed=None, outliers=False):
    """synthetic_msckf inputs of the issue's seeds (0xE4F0 + k); outliers: z[2r] += 25 on 1 - 3 blocks per filter, as
    synthetic_ekf does."""
    s = sc.synthetic_msckf(B, k, m=m, seed=0xE4F0 + k if seed is None else seed)
    s["P"] = s["P"].reshape(B, s["N"], s["N"])
    if outliers:
        rng = np.random.default_rng(s["N"] * 1000 + m)
        for b in range(B):
            for r in rng.choice(m // 2, size=1 + b % 3, replace=False):
                s["z"][b, 2 * r] += 25.0
    return s


def gate_d2(k, mean_b, P_b, z_b, zmean_b, H_b, R):
    """Every d2 the gate of the EKF update decides on for one filter (the numpy twin's walk of removeOutliers)."""
    from oracle import np_check as npc
    d2 = []
    npc.msckf_update_ekf(npc.Msckf(k, mean_b, P_b), z_b, zmean_b, H_b, R, decisions=d2)
    return np.array(d2, dtype=np.float64)


def rank_premise(H_b):
    """(rank, number of distinct observed poses, sigma_min / sigma_max) over the non-zero columns of one filter's H."""
    nz = np.abs(H_b).max(axis=0) > 0
    sv = np.linalg.svd(H_b[:, nz], compute_uv=False)
    return int(np.linalg.matrix_rank(H_b)), int(nz.sum()) // 6, float(sv.min() / sv.max())
