"""Msckf EKF update (slk_update_ekf, Msckf.hpp:284-349) on both kernels that serve it, against the CPU oracle run one
filter at a time and against the textbook update.

slk_update_ekf runs msckf_ekf_tile_kernel (slk_ekf_tiles.hpp: 16 x 16 LDS tiles, m <= 128 and N <= 64) or
msckf_ekf_kernel (slk_ekf.hpp: global workspace, every other shape up to m = 512).  Covered here: the tile geometry
(N = 12 .. 60, square thinQ, zero-column and dense full-rank Jacobians), the same filters on both sides of the route
boundary, the general kernel at m = 512, gate decisions pinned by place, per-filter isolation in one launch, full
batches, the device-tensor route, a shared R, the wrapper's refusals and the hand-off to a fused step.  Status and
outlier counts must be equal; P and the mean (by boxminus) within TOL relative; a filter the update was not applied to
keeps its state bit for bit.  Run with `pytest -m gpu` on an MI355X (`-s` prints the worst error seen per kernel)."""
import numpy as np
import pytest

from oracle import np_check as npc
from oracle import oracle as o
import scenarios as sc

pytestmark = pytest.mark.gpu

TOL = 1e-9
CHI2 = 5.99                                   # the gate's threshold, chi2_0.95(2) (Msckf.hpp:861-865)
WORST = {"tile": [0.0, 0.0], "general": [0.0, 0.0]}      # worst relative error of P / of the mean, per kernel


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    yield mod
    for kern, (ep, em) in WORST.items():
        print(f"\nEKF {kern} kernel: worst relative error P {ep:.2e}, mean {em:.2e}")


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def mean_err(lay, a, b):
    return float(np.abs(o.boxminus(lay, a, b)).max())


def kernel(N, m):
    """The kernel slk_update_ekf launches for this shape."""
    return "tile" if m <= 128 and N <= 64 else "general"


def gpu(slk, e, z=None, H=None, R=None, gate=True):
    """One launch over the whole batch -> (status, outliers, P, mean)."""
    f = slk.Msckf(e["mean"], e["P"])
    f.update_ekf(e["z"] if z is None else z, e["zmean"], e["H"] if H is None else H, e["R"] if R is None else R,
                 gate=gate)
    return f.status(), f.outliers(), f.getPk(), f.muState()


def note(N, m, ep, em):
    w = WORST[kernel(N, m)]
    w[0], w[1] = max(w[0], ep), max(w[1], em)


def check(e, res, z=None, H=None, R=None, gate=True, filters=None):
    """Each filter (or each of `filters`) against the oracle run of that filter alone: status and outliers equal; where
    the update was applied, P and the mean within TOL (NaN in the same places) and, on the tile kernel, P exactly
    symmetric; elsewhere the state bit-identical to the input.  Returns the filters the update was applied to."""
    st, out, P, M = res
    z = e["z"] if z is None else z
    H = e["H"] if H is None else H
    R = e["R"] if R is None else R
    k, N, m = e["k"], e["N"], z.shape[-1]
    lay = o.layout(o.MULTI, k)
    applied = []
    for b in range(len(st)) if filters is None else filters:
        r = o.Msckf(k, e["mean"][b], e["P"][b])
        sto, no = r.update_ekf(z[b], e["zmean"][b], H[b], R if R.ndim == 2 else R[b], gate=gate)
        assert (st[b], out[b]) == (sto, no), (b, st[b], sto, out[b], no)
        if sto == 0 and no < m // 2:
            nan = np.isnan(r.mean)
            np.testing.assert_array_equal(np.isnan(M[b]), nan)
            ep = rel(P[b], r.P)
            em = 0.0 if nan.any() else mean_err(lay, M[b], r.mean)
            assert ep <= TOL and em <= TOL, (b, ep, em)
            note(N, m, ep, em)
            if kernel(N, m) == "tile":
                assert np.array_equal(P[b], P[b].T), b
            applied.append(b)
        else:
            assert np.array_equal(P[b], e["P"][b]) and np.array_equal(M[b], e["mean"][b]), b
    return applied


def gate_margin(e, z=None, R=None, filters=None):
    """Smallest relative distance from the threshold of any d2 that decides a pair (numpy S0^-1 and the numpy twin's
    walk of the gate): above 1e-6, Cholesky and LU rounding cannot flip a decision.  A NaN d2 is rejected whatever the
    rounding."""
    z = e["z"] if z is None else z
    R = e["R"] if R is None else R
    d2 = []
    for b in range(e["B"]) if filters is None else filters:
        h = npc.Msckf(e["k"], e["mean"][b], e["P"][b])
        npc.msckf_update_ekf(h, z[b], e["zmean"][b], e["H"][b], R if R.ndim == 2 else R[b], decisions=d2)
    d2 = np.array(d2)
    d2 = d2[np.isfinite(d2)]
    return float(np.abs(d2 - CHI2).min() / CHI2) if d2.size else np.inf


def with_outliers(e, seed):
    """z with outliers in min(b, (m - N) / 2) random pairs of filter b, on either row of the pair (one on the second row
    is re-tested after the shifted erase): more than N rows survive on most filters."""
    rng = np.random.default_rng(seed)
    z = e["z"].copy()
    m, N = e["m"], e["N"]
    for b in range(e["B"]):
        for p in rng.choice(m // 2, size=min(b, (m - N) // 2), replace=False):
            z[b, 2 * p + int(rng.integers(2))] += 25.0
    return z


# ------------------------------------------------------------------ a. tile kernel sweep
def _sweep():
    for k in range(9):
        N = 12 + 6 * k
        for m in sorted({N, N + 2, -(-(N + 2) // 16) * 16, 126, 128}):
            yield k, m


@pytest.mark.parametrize("dense", [False, True], ids=["zero_cols", "dense"])
@pytest.mark.parametrize("k,m", list(_sweep()))
def test_ekf_tile_kernel_sweep(slk, k, m, dense):
    # every N = 12 .. 60 the tile kernel holds (one to four column tiles, N = 48 tile-exact), m from N (square thinQ:
    # the last reflector has an empty tail) to 128 (eight row tiles, lane 63 of the gate's ballot); gate on and off
    B = 4
    e = sc.synthetic_ekf(B, k, m, seed=0x7113 + 97 * k + m, outliers=False, dense=dense)
    assert kernel(e["N"], m) == "tile"
    z = with_outliers(e, seed=31 * k + m)
    assert gate_margin(e, z=z) > 1e-6
    assert check(e, gpu(slk, e, z=z), z=z), "no filter took the update"
    assert len(check(e, gpu(slk, e, gate=False), gate=False)) == B


# ------------------------------------------------------------------ b. route boundary and general-kernel extremes
def test_ekf_same_filters_on_both_sides_of_the_route_boundary(slk):
    # N = 60: m = 128 is the tile kernel's largest row count, m = 130 the general kernel's next one
    e = sc.synthetic_ekf(4, 8, 130, seed=0xB0DE, dense=True)
    t = dict(e, m=128, z=np.ascontiguousarray(e["z"][:, :128]), zmean=np.ascontiguousarray(e["zmean"][:, :128]),
             H=np.ascontiguousarray(e["H"][:, :128]), R=np.ascontiguousarray(e["R"][:, :128, :128]))
    assert kernel(60, 128) == "tile" and kernel(60, 130) == "general"
    for x in (t, e):
        assert len(check(x, gpu(slk, x))) == 4
    # m = 128 at N = 60 (tile kernel) and at N = 66 (general kernel)
    assert kernel(66, 128) == "general"
    for k in (8, 9):
        x = sc.synthetic_ekf(4, k, 128, seed=0xB1DE + k, dense=True)
        assert len(check(x, gpu(slk, x))) == 4


@pytest.mark.parametrize("k", [9, 33])
def test_ekf_general_kernel_at_512_rows(slk, k):
    # the largest m the library takes (the gate's row list idx[520]), at N = 66 and N = 210, gated
    e = sc.synthetic_ekf(2, k, 512, seed=0x5120 + k, dense=True)
    assert len(check(e, gpu(slk, e))) == 2


def test_ekf_row_counts_the_library_refuses(slk):
    for k, ms in ((8, (514, 127, 58)), (9, (514, 81, 64))):
        e = sc.synthetic_ekf(2, k, 80, seed=0x0DD + k)
        N = e["N"]
        f = slk.Msckf(e["mean"], e["P"])
        for m in ms:                          # more than 512, odd, fewer than N
            with pytest.raises(slk.SlkError):
                f.update_ekf(np.zeros((2, m)), np.zeros((2, m)), np.zeros((2, m, N)), np.eye(m))
        assert (f.status() == 0).all() and np.array_equal(f.getPk(), e["P"]) and np.array_equal(f.muState(), e["mean"])


# ------------------------------------------------------------------ c. gate edges
@pytest.mark.parametrize("case", sc.EKF_EDGE_CASES)
@pytest.mark.parametrize("m", [128, 160])
def test_ekf_gate_edges(slk, m, case):
    # N = 60; m = 128 runs the tile kernel (its ballot's lane 63 is the last pair), m = 160 the general kernel
    B = 3
    e = sc.ekf_gate_edge(B, 8, m, case, seed=0xED6E + m)
    N = e["N"]
    assert gate_margin(e) > 1e-6
    st, out, P, M = res = gpu(slk, e)
    left = m - 2 * e["n_out"]
    assert (out == e["n_out"]).all(), (out, e["n_out"])
    assert (st == (slk.ST_EKF_ROWS if 0 < left < N else 0)).all(), st
    assert len(check(e, res)) == (B if left >= N else 0)


# ------------------------------------------------------------------ d. known answers
@pytest.mark.parametrize("k,m,iso", [(8, 60, False), (8, 128, True), (9, 80, True), (9, 66, False)])
def test_ekf_textbook_update(slk, k, m, iso):
    # gate off, dense H of full column rank: m = N (thinQ square, any SPD R carries over exactly) or R = s^2 I (the
    # compression is lossless) -- the result is P - K S K^T and mu [+] K (z - zmean), S = H P H^T + R, K = P H^T S^-1
    B = 3
    e = sc.synthetic_ekf(B, k, m, seed=0x7E47 + k + m, outliers=False, dense=True)
    if iso:
        e["R"] = np.ascontiguousarray(np.broadcast_to(0.04 * np.eye(m), (B, m, m)))
    st, out, P, M = gpu(slk, e, gate=False)
    assert (st == 0).all() and (out == 0).all()
    lay = o.layout(o.MULTI, k)
    man = npc.Manifold.multi(k)
    for b in range(B):
        Hb, Pb = e["H"][b], e["P"][b]
        S = Hb @ Pb @ Hb.T + e["R"][b]
        K = Pb @ Hb.T @ np.linalg.inv(S)
        mu = man.plus(e["mean"][b], K @ (e["z"][b] - e["zmean"][b]))
        ep, em = rel(P[b], Pb - K @ S @ K.T), mean_err(lay, M[b], mu)
        assert ep <= TOL and em <= TOL, (b, ep, em)
        note(e["N"], m, ep, em)


# ------------------------------------------------------------------ e. per-filter isolation in one launch
@pytest.mark.parametrize("m", [128, 160])
def test_ekf_per_filter_isolation(slk, m):
    # one batch mixing every outcome: normal filters (0, 1, 3, 7; 1 and 3 with an outlier), an indefinite R (2), N - 2
    # rows left (4), every pair rejected (5), a NaN in z (6): each filter is the oracle's run of it alone, and the normal
    # ones are bit-identical to a batch without the odd ones
    B, k = 8, 8
    e = sc.synthetic_ekf(B, k, m, seed=0x150 + m, outliers=False, dense=True)
    N = e["N"]
    z0 = e["zmean"] + np.random.default_rng(m).normal(0, 0.01, (B, m))
    z0[1, 0] += 25.0
    z0[3, m - 1] += 25.0
    R0 = e["R"]
    z, R = z0.copy(), R0.copy()
    R[2] = -np.eye(m)
    z[4, sc.ekf_outlier_rows("rows_N-2", m, N)[0]] += 25.0
    z[5] += 25.0
    z[6, 10] = np.nan
    normal = [0, 1, 3, 7]
    assert gate_margin(e, z=z, filters=[0, 1, 3, 4, 5, 6, 7]) > 1e-6
    clean = gpu(slk, e, z=z0, R=R0)
    odd = gpu(slk, e, z=z, R=R)
    st, out, P, M = odd
    # an indefinite R: S0 = H P H^T + R is not SPD, the Cholesky reports it and the filter is left alone (the oracle
    # inverts it with partial-pivot LU, like the reference, and goes on: DESIGN.md section 7)
    assert st[2] == slk.ST_SINGULAR and out[2] == 0
    assert np.array_equal(P[2], e["P"][2]) and np.array_equal(M[2], e["mean"][2])
    assert check(e, odd, z=z, R=R, filters=[0, 1, 3, 4, 5, 6, 7]) == [0, 1, 3, 6, 7]
    assert st[4] == slk.ST_EKF_ROWS and st[5] == 0 and out[5] == m // 2 and out[6] == 1
    for a, c in zip(odd, clean):
        np.testing.assert_array_equal(a[normal], c[normal])
    # ungated, the NaN reaches filter 6's mean (and nothing else)
    zn = z0.copy()
    zn[6, 10] = np.nan
    clean = gpu(slk, e, z=z0, gate=False)
    odd = gpu(slk, e, z=zn, gate=False)
    assert len(check(e, odd, z=zn, gate=False)) == B
    assert np.isnan(odd[3][6]).any() and not np.isnan(odd[2][6]).any()
    keep = [b for b in range(B) if b != 6]
    for a, c in zip(odd, clean):
        np.testing.assert_array_equal(a[keep], c[keep])


# ------------------------------------------------------------------ f. full batches
@pytest.mark.parametrize("B,k,m", [(1024, 8, 128), (256, 9, 80)], ids=["tile", "general"])
def test_ekf_full_batch(slk, B, k, m):
    # every filter's status and outliers against the oracle's, 32 sampled filters at TOL; the tile kernel's P symmetric
    e = sc.synthetic_ekf(B, k, m, seed=0xFB00 + m, dense=True)
    st, out, P, M = res = gpu(slk, e)
    for b in range(B):
        r = o.Msckf(k, e["mean"][b], e["P"][b])
        sto, no = r.update_ekf(e["z"][b], e["zmean"][b], e["H"][b], e["R"][b])
        assert (st[b], out[b]) == (sto, no), (b, st[b], sto, out[b], no)
    assert out.sum() > 0
    sample = sorted(np.random.default_rng(B).choice(B, 32, replace=False).tolist())
    assert len(check(e, res, filters=sample)) >= 24
    if kernel(e["N"], m) == "tile":
        assert np.array_equal(P, np.transpose(P, (0, 2, 1)))


# ------------------------------------------------------------------ g. routes, refusals and hand-off
@pytest.mark.parametrize("k,m", [(8, 128), (9, 80)], ids=["tile", "general"])
def test_ekf_device_tensors_and_shared_R_match_the_host_route(slk, k, m):
    import torch
    B = 6
    e = sc.synthetic_ekf(B, k, m, seed=0x6E0 + m, dense=True)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    Hd = d(np.transpose(e["H"], (0, 2, 1)))                              # [B, N, m]: m x N column-major per filter
    host = gpu(slk, e)
    check(e, host)
    f = slk.Msckf(e["mean"], e["P"])
    f.update_ekf(d(e["z"]), d(e["zmean"]), Hd, d(np.transpose(e["R"], (0, 2, 1))))
    for a, c in zip((f.status(), f.outliers(), f.getPk(), f.muState()), host):
        np.testing.assert_array_equal(a, c)
    # one R [m, m] shared by the batch against the same R tiled per filter, on both routes
    R0 = e["R"][0]
    shared = gpu(slk, e, R=R0)
    check(e, shared, R=R0)
    for a, c in zip(gpu(slk, e, R=np.ascontiguousarray(np.broadcast_to(R0, (B, m, m)))), shared):
        np.testing.assert_array_equal(a, c)
    f = slk.Msckf(e["mean"], e["P"])
    f.update_ekf(d(e["z"]), d(e["zmean"]), Hd, d(R0.T))
    for a, c in zip((f.status(), f.outliers(), f.getPk(), f.muState()), shared):
        np.testing.assert_array_equal(a, c)


def test_ekf_wrapper_refuses_mixed_sides_and_bad_tensors(slk):
    # the refusals happen before any library call: slk_update_ekf is swapped for a trap, so no host address ever
    # reaches the kernel as a device pointer
    import torch

    class Trap:
        def __init__(self, lib):
            self.lib = lib

        def __getattr__(self, name):
            if name == "slk_update_ekf":
                pytest.fail("slk_update_ekf called with arguments the wrapper must refuse")
            return getattr(self.lib, name)

    B, k, m = 2, 8, 64
    e = sc.synthetic_ekf(B, k, m, seed=0x7AB, outliers=False)
    dev = torch.device("cuda", 0)
    Rt = np.ascontiguousarray(np.transpose(e["R"], (0, 2, 1)))
    z, zm = torch.from_numpy(e["z"]).to(dev), torch.from_numpy(e["zmean"]).to(dev)
    H = torch.from_numpy(np.ascontiguousarray(np.transpose(e["H"], (0, 2, 1)))).to(dev)
    R = torch.from_numpy(Rt).to(dev)
    f = slk.Msckf(e["mean"], e["P"])
    lib = f._lib
    f._lib = Trap(lib)
    bad = [(z, zm, H, e["R"]),                                 # numpy R next to device tensors
           (z, zm, H, torch.from_numpy(Rt)),                   # a CPU tensor R
           (z, zm, H.cpu(), R),                                # a CPU tensor H
           (e["z"], e["zmean"], H, R),                         # numpy z, zmean next to a device H
           (z, zm, H.float(), R),                              # float32 H
           (z.float(), zm, H, R),                              # float32 z
           (z, zm, H, R.float()),                              # float32 R
           (z, zm, H[:, :, :m - 2].contiguous(), R),           # H of the wrong size
           (z, zm, H.transpose(1, 2), R),                      # H not contiguous
           (z, zm, H, R[:, :m // 2, :m // 2].contiguous())]    # R of the wrong size
    for args in bad:
        with pytest.raises(slk.SlkError):
            f.update_ekf(*args)
    f._lib = lib
    assert (f.status() == 0).all() and np.array_equal(f.getPk(), e["P"]) and np.array_equal(f.muState(), e["mean"])
    f.update_ekf(z, zm, H, R)
    assert len(check(e, (f.status(), f.outliers(), f.getPk(), f.muState()))) == B


@pytest.mark.parametrize("m", [128, 130], ids=["tile", "general"])
def test_ekf_then_fused_step_matches_the_oracle(slk, m):
    # the fused step reads only the lower triangle of P; the general kernel leaves a P that is not bit-symmetric
    B, k = 4, 8
    seed = 0x5E9 + m
    e = sc.synthetic_ekf(B, k, m, seed=seed, dense=True)
    s = sc.synthetic_msckf(B, k, m=8, seed=seed)         # the same filters, with a process input and four features
    assert np.array_equal(s["mean"], e["mean"])
    f = slk.Msckf(e["mean"], e["P"])
    f.update_ekf(e["z"], e["zmean"], e["H"], e["R"])
    st1, out1 = f.status(), f.outliers()
    assert (st1 == 0).all()
    f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    out2, P, M = f.outliers(), f.getPk(), f.muState()
    assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
    lay = o.layout(o.MULTI, k)
    for b in range(B):
        r = o.Msckf(k, e["mean"][b], e["P"][b])
        sto, no = r.update_ekf(e["z"][b], e["zmean"][b], e["H"][b], e["R"][b])
        assert sto == 0 and no == out1[b], (b, sto, no, out1[b])
        u = s["u"][b]
        assert r.predict(o.pm_delta_pose(u[0:3], u[3:7], u[7:10], u[10:13]), s["Q"]) == 0
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto & ~slk.ST_ALL_REJECTED == 0 and no == out2[b], (b, sto, no, out2[b])
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b
