"""Numpy twin of the Msckf feature-track update (slk_track_linearize) and the inputs its tests share.  The twin follows
the steps of include/slk.h one by one -- the same linear start, the same five Gauss-Newton iterations, the same flags --
but takes its null space from np.linalg.qr(H_f, mode="complete")[:, 3:], a different basis from the kernel's three
reflectors on purpose: what is compared across the two is basis-independent (H^T H, H^T r, r^T r, gamma, the posterior).
No product; the oracle is not needed here."""
import numpy as np

import scenarios as sc
from ekf_model_ref import quat_matrix, skew

SIGMA = 0.01
SHAPES = [(2, 3, 8, 24), (8, 9, 4, 60), (8, 9, 5, 76), (8, 5, 10, 128), (9, 4, 14, 70), (31, 32, 4, 244)]   # (k, M, J, m)
IDS = [f"k{k}-M{M}-J{J}-m{m}" for k, M, J, m in SHAPES]
# chi-square 0.95 quantiles by degrees of freedom 0 .. 61 (Wilson-Hilferty; the level is the caller's, any table does)
CHI2_95 = np.array([0.0] + [d * (1 - 2 / (9 * d) + 1.6448536269514722 * np.sqrt(2 / (9 * d))) ** 3 for d in range(1, 62)])


def pose_offsets(c):
    """storage offset, tangent offset of pose index c (0 = the state, c >= 1 = clone c - 1)"""
    return (0, 0) if c == 0 else (13 + 7 * (c - 1), 12 + 6 * (c - 1))


def solve3(A, b):
    """x = A^-1 b by the 3 x 3 Cholesky of the kernel; ok False for a non-positive or NaN pivot"""
    with np.errstate(all="ignore"):
        ok = bool(A[0, 0] > 0)
        l00 = np.sqrt(A[0, 0]); l10 = A[1, 0] / l00; l20 = A[2, 0] / l00
        d1 = A[1, 1] - l10 * l10
        ok = ok and bool(d1 > 0)
        l11 = np.sqrt(d1); l21 = (A[2, 1] - l20 * l10) / l11
        d2 = A[2, 2] - l20 * l20 - l21 * l21
        ok = ok and bool(d2 > 0)
        l22 = np.sqrt(d2)
        y0 = b[0] / l00; y1 = (b[1] - l10 * y0) / l11; y2 = (b[2] - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00
    return np.array([x0, x1, x2]), ok


def project(Rt, p, X):
    """l = R^T (X - p), J = d pi / d l, F = J R^T"""
    l = Rt @ (X - p)
    with np.errstate(all="ignore"):
        J = np.array([[1 / l[2], 0, -l[0] / l[2] ** 2], [0, 1 / l[2], -l[1] / l[2] ** 2]])
    return l, J, J @ Rt


def triangulate(mean_b, track):
    """Steps 1 - 3 for one track [M, 3]: (X, flag, observed slots); flag 1 = triangulated, 0 = unused, -1 = failed."""
    obs = [(s, int(c)) for s, c in enumerate(track[:, 0]) if c >= 0]
    if len(obs) < 2:
        return np.zeros(3), 0, obs
    if len({c for _, c in obs}) < len(obs):
        return np.full(3, np.nan), -1, obs
    A, bv, poses = np.zeros((3, 3)), np.zeros(3), []
    for s, c in obs:
        sp, _ = pose_offsets(c)
        p, R = mean_b[sp:sp + 3], quat_matrix(mean_b[sp + 3:sp + 7])
        d = R @ np.array([track[s, 1], track[s, 2], 1.0])
        d = d / np.sqrt(d @ d)
        Mi = np.eye(3) - np.outer(d, d)
        A += Mi
        bv += Mi @ p
        poses.append((p, R.T, track[s, 1:3]))
    X, ok = solve3(A, bv)
    with np.errstate(all="ignore"):
        for _ in range(5):
            G, g = np.zeros((3, 3)), np.zeros(3)
            for p, Rt, uv in poses:
                l, _, F = project(Rt, p, X)
                G += F.T @ F
                g += F.T @ (l[:2] / l[2] - uv)
            d, okd = solve3(G, g)
            ok = ok and okd
            X = X - d
        depth_ok = all(project(Rt, p, X)[0][2] > 0 for p, Rt, _ in poses)
    if not ok or not np.isfinite(X).all() or not depth_ok:
        return np.full(3, np.nan), -1, obs
    return X, 1, obs


def blocks(mean_b, track, X, obs, k):
    """Step 4: r [2M], H_x [2M, N], H_f [2M, 3] of one track at X, empty slots zero rows."""
    M, N = track.shape[0], 12 + 6 * k
    r, Hx, Hf = np.zeros(2 * M), np.zeros((2 * M, N)), np.zeros((2 * M, 3))
    for s, c in obs:
        sp, tp = pose_offsets(c)
        l, J, F = project(quat_matrix(mean_b[sp + 3:sp + 7]).T, mean_b[sp:sp + 3], X)
        r[2 * s:2 * s + 2] = track[s, 1:3] - l[:2] / l[2]
        Hx[2 * s:2 * s + 2, tp:tp + 3] = -F
        Hx[2 * s:2 * s + 2, tp + 3:tp + 6] = J @ skew(l)
        Hf[2 * s:2 * s + 2] = F
    return r, Hx, Hf


def lower(P_b):
    """P as the kernels read it: from its lower triangle only"""
    return np.tril(P_b) + np.tril(P_b, -1).T


def linearize_np(mean_b, P_b, tracks_b, sigma, k, m, chi2=None, rotate=None):
    """One filter: r [m], H [m, N], feat [J, 4], gamma [J] (NaN where no gate was evaluated).  rotate: a generator that
    multiplies each track's rows by a random orthogonal matrix (the basis-independence check)."""
    J, M = tracks_b.shape[:2]
    N, nr = 12 + 6 * k, 2 * M - 3
    r, H, feat, gamma = np.zeros(m), np.zeros((m, N)), np.zeros((J, 4)), np.full(J, np.nan)
    Pl = lower(P_b)
    for j in range(J):
        X, flag, obs = triangulate(mean_b, tracks_b[j])
        if flag == 1:
            rr, Hx, Hf = blocks(mean_b, tracks_b[j], X, obs, k)
            Nn = np.linalg.qr(Hf, mode="complete")[0][:, 3:]
            if rotate is not None:
                Nn = Nn @ np.linalg.qr(rotate.normal(size=(nr, nr)))[0]
            rj, Hj = Nn.T @ rr / sigma, Nn.T @ Hx / sigma
            if chi2 is not None:
                gamma[j] = rj @ np.linalg.solve(Hj @ Pl @ Hj.T + np.eye(nr), rj)
                if not gamma[j] < chi2[2 * len(obs) - 3]:
                    flag = -2
            if flag == 1:
                r[j * nr:(j + 1) * nr], H[j * nr:(j + 1) * nr] = rj, Hj
        feat[j, :3], feat[j, 3] = X, flag
    return r, H, feat, gamma


def linearize_batch(s, chi2=None, rotate=None):
    """Every filter of a scenario: r [B, m], H [B, m, N], feat [B, J, 4], gamma [B, J]"""
    out = [linearize_np(s["mean"][b], s["P"][b], s["tracks"][b], s["sigma"], s["k"], s["m"], chi2, rotate) for b in range(s["B"])]
    return tuple(np.stack(x) for x in zip(*out))


def observe(mean_b, X, c, rng=None, sigma=SIGMA):
    """(u, v) of the world point X from pose c of one filter, with N(0, sigma^2) noise"""
    sp, _ = pose_offsets(c)
    l = quat_matrix(mean_b[sp + 3:sp + 7]).T @ (X - mean_b[sp:sp + 3])
    uv = l[:2] / l[2]
    return uv if rng is None else uv + rng.normal(0, sigma, 2)


_CACHE = {}


def scenario(k, M, J, m, B=4, seed=None, shared=False):
    """synthetic_msckf poses (the mean is the truth), landmarks 3 - 8 units in front of the window, projected into the
    observing poses with N(0, SIGMA^2) noise.  M == k + 1: every pose observes every track; otherwise each track is seen
    from 3 .. M poses drawn at random, in random slots, the other slots empty (c = -1).  shared: every filter carries
    filter 0's poses, its position moved by 1e-3, and filter 0's tracks.  Cached: treat the arrays as read-only."""
    key = (k, M, J, m, B, seed, shared)
    if key in _CACHE:
        return dict(_CACHE[key])
    sd = 0x7AC0 + 16 * k + M if seed is None else seed
    s = sc.synthetic_msckf(B, k, m=8, seed=sd)
    rng = np.random.default_rng(sd + 1)
    mean = s["mean"].copy()
    if shared:
        mean[:] = mean[0]
        for c in range(k + 1):
            sp, _ = pose_offsets(c)
            mean[1:, sp:sp + 3] += rng.normal(0, 1e-3, (B - 1, 3))
    tracks = np.zeros((B, J, M, 3))
    tracks[..., 0] = -1.0
    land = np.zeros((B, J, 3))
    for b in range(B):
        R0 = quat_matrix(mean[b, 3:7])
        for j in range(J):
            land[b, j] = mean[b, 0:3] + R0 @ np.concatenate([rng.uniform(-1, 1, 2), rng.uniform(3, 8, 1)])
            n = M if M == k + 1 else int(rng.integers(min(3, M), M + 1))
            poses = rng.choice(k + 1, size=n, replace=False)
            slots = np.sort(rng.choice(M, size=n, replace=False))
            for sl, c in zip(slots, poses):
                tracks[b, j, sl, 0] = c
                tracks[b, j, sl, 1:3] = observe(mean[b], land[b, j], int(c), rng)
    if shared:
        tracks[:] = tracks[0]
        land[:] = land[0]
    out = dict(B=B, k=k, M=M, J=J, m=m, N=s["N"], Nq=s["Nq"], mean=np.ascontiguousarray(mean),
               P=np.ascontiguousarray(s["P"].reshape(B, s["N"], s["N"])), tracks=tracks, land=land, sigma=SIGMA, u=s["u"], Q=s["Q"],
               ukf=dict(z=s["z"], feat=s["feat"].reshape(B, -1), R=s["R"]))
    _CACHE[key] = out
    return dict(out)


def flag_scenario():
    """(8, 5, 10, 128) with one track of each kind in filter 1: 0 one observation, 1 all slots empty, 2 a pose named
    twice, 3 the image points of the landmark's mirror image, 4 one observation moved by 25 sigma.  P is a hundredth of the
    scenario's: with its 0.1 rad of attitude uncertainty a 25 sigma residual would pass the gate."""
    k, M, J, m = SHAPES[3]
    s = scenario(k, M, J, m)
    t = s["tracks"].copy()
    b = 1
    t[b, 0, :, 0] = -1.0
    t[b, 0, 2] = (3.0, 0.1, -0.2)
    t[b, 1, :, 0] = -1.0
    t[b, 2, :, 0] = (1.0, 4.0, -1.0, 4.0, 6.0)
    mirror = 2 * s["mean"][b, 0:3] - s["land"][b, 3]
    for sl, c in enumerate((0, 2, 5, 7, 8)):
        t[b, 3, sl, 0] = c
        t[b, 3, sl, 1:3] = observe(s["mean"][b], mirror, c)
    for sl, c in enumerate((0, 2, 4, 6, 8)):
        t[b, 4, sl, 0] = c
        t[b, 4, sl, 1:3] = observe(s["mean"][b], s["land"][b, 4], c, np.random.default_rng(5 + sl))
    t[b, 4, 2, 2] += 25 * s["sigma"]
    s = dict(s, P=1e-2 * s["P"])
    s2 = dict(s, tracks=t)
    return s, s2, b
