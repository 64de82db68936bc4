"""The exact-shape Msckf update (k = 4 .. 8, m = 8; csrc/slk_step_fast.hpp) starts Z = h(X) under the tail of the first
factorisation: wave 0 factors the covariance panel by panel and, behind the tile stores of step ksmax = jmax >> 2 (jmax = the last
sigma column any measurement row depends on: a feature on pose c reads the rows tp .. tp + 5 of the factor at the columns
j <= tp + 5, tp = 0 or 6 + 6 c), meets the other three waves in one barrier; they evaluate their features while wave 0 runs its
remaining steps.  The conditions that hand a filter to the general body (failed factorisation, pose index, rotation bound,
the exponential's domain) are decided in the barrier that closes h(X), so h(X) also runs on filters that are about to leave.

What that could lose is checked against the oracle's batch step at the smallest shapes where it can go wrong:

  * k = 8, all four features on one pose c = 0 .. 8: the release behind step 1, 4, 5, 7, 8, 10, 11, 13 and, at c = 8, at the end
    of the factorisation (step 14);
  * the other instantiations: k = 4 (nine steps) with c = 0, 2, 4, and one case each for k = 5, 6, 7;
  * the maximum decides: [0, 0, 0, 5], [4, 1, 1, 1], a batch whose filters differ (one on the newest pose beside early ones),
    and batches of 1 and 7 filters;
  * the gate: one and two blocks pushed out on an early-release filter;
  * a covariance that is not positive definite, the first bad pivot before, at and after the release column (a negative
    diagonal entry at row 2, at jmax = 35, at row 50): SLK_ST_LLT_FAIL as the oracle's LLT reports, the state kept bit for
    bit, the neighbours in parity with the oracle;
  * filters that leave the fast path after an early h(X): a rotation column beyond 4 rad on an observed clone (the
    exponential of h(X) raises its flag on a waiting wave), a pose index of K + 1 and of -1 on the features 1 .. 3 in
    device-resident parameters (SLK_ST_BAD_INDEX, clamped before it forms an address) -- the general body's result.
Every case: outliers equal to the oracle's, P exactly symmetric.  B = 8 filters, 3 steps; TOL = 1e-9 and the helpers of
tests/test_gpu_routes.py, the scenario builder of tests/test_gpu_live_column_bound.py.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
from test_gpu_live_column_bound import last_live_column, scenario
from test_gpu_routes import TOL, colmajor_P, mean_err, rel

pytestmark = pytest.mark.gpu
STEPS, M = 3, 8
BAD = 2                                                          # the filter of a batch that is damaged


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def release_step(poses):
    """The step of the factorisation (four columns each) behind which h(X) may start: the one that holds column jmax."""
    return last_live_column(poses) >> 2


def first_filters(s, n):
    """The first n filters of a scenario (the builder makes eight)."""
    t = dict(s)
    for name in ("mean", "P", "u", "feat", "z"):
        t[name] = np.ascontiguousarray(s[name][:n])
    t["B"] = n
    return t


def run_and_compare(slk, s, label, P=None, any_rejected_status=False):
    """STEPS fused steps against the oracle's batch step: status, outliers, P and mean of every filter, P exactly symmetric."""
    k, N, lay = s["k"], s["N"], o.layout(o.MULTI, s["k"])
    P = s["P"] if P is None else P
    n = P.shape[0]
    f = slk.Msckf(s["mean"], P)
    tot = np.zeros(n, dtype=np.int64)
    for _ in range(STEPS):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += f.outliers()
    st = f.status()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(n, -1)
    sto, oc = o.msckf_step_batch(k, M, STEPS, om, oP, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    oP = colmajor_P(oP, N)
    Pg, Mg = f.getPk(), f.muState()
    errs = [(rel(Pg[b], oP[b]), mean_err(lay, Mg[b], om[b])) for b in range(n)]
    print(f"k={k} B={n} {label}: status {st}, outliers {tot} / oracle {oc}, worst P {max(e[0] for e in errs):.2e}, "
          f"mean {max(e[1] for e in errs):.2e}")
    assert sto == 0
    if any_rejected_status:
        assert (st & ~slk.ST_ALL_REJECTED == 0).all()
    else:
        assert (st == 0).all()
    np.testing.assert_array_equal(tot, oc)
    for b in range(n):
        assert errs[b][0] <= TOL and errs[b][1] <= TOL, (b, errs[b])
        np.testing.assert_array_equal(Pg[b], Pg[b].T)
    return oc


# ------------------------------------------------------------------ the release behind every step it can stand behind
@pytest.mark.parametrize("c", list(range(9)))
def test_k8_release_behind_each_step(slk, c):
    poses = [c] * 4
    assert release_step(poses) == (1, 4, 5, 7, 8, 10, 11, 13, 14)[c]      # c = 8: the last of the fifteen steps
    run_and_compare(slk, scenario(8, poses), f"poses {poses} (release behind step {release_step(poses)})")


@pytest.mark.parametrize("c", [0, 2, 4])
def test_k4_release(slk, c):
    poses = [c] * 4
    assert release_step(poses) == {0: 1, 2: 5, 4: 8}[c] and (c != 4 or last_live_column(poses) == 12 + 6 * 4 - 1)
    run_and_compare(slk, scenario(4, poses), f"poses {poses} (release behind step {release_step(poses)})")


@pytest.mark.parametrize("k,poses,step", [(5, [2, 2, 2, 2], 5), (6, [3, 1, 0, 2], 7), (7, [4, 4, 0, 4], 8)])
def test_k5_k6_k7_release(slk, k, poses, step):
    assert release_step(poses) == step and step < (12 + 6 * k - 1) >> 2   # an early release in every one of them
    run_and_compare(slk, scenario(k, poses), f"poses {poses} (release behind step {step})")


# ------------------------------------------------------------------ the maximum over a filter's features decides
@pytest.mark.parametrize("poses,step", [([0, 0, 0, 5], 10), ([4, 1, 1, 1], 8)])
def test_mixed_poses_the_maximum_decides(slk, poses, step):
    assert release_step(poses) == step
    run_and_compare(slk, scenario(8, poses, seed_tag=1 + poses[0]), f"poses {poses} (release behind step {step})")


PER_FILTER = [[0, 0, 0, 0], [1, 1, 1, 1], [4, 1, 1, 1], [0, 0, 0, 5], [8, 8, 8, 8], [2, 7, 2, 2], [3, 3, 3, 3], [6, 0, 6, 0]]


def test_filters_of_one_batch_release_at_different_steps(slk):
    assert [release_step(p) for p in PER_FILTER] == [1, 4, 8, 10, 14, 13, 7, 11]       # filter 4: the newest pose, at the end
    run_and_compare(slk, scenario(8, PER_FILTER, seed_tag=9), "poses per filter")


@pytest.mark.parametrize("n", [1, 7])
def test_small_batches(slk, n):
    s = first_filters(scenario(8, PER_FILTER, seed_tag=9), n)
    run_and_compare(slk, s, "poses per filter")


# ------------------------------------------------------------------ the gate on an early-release filter
@pytest.mark.parametrize("nrej", [1, 2])
def test_rejected_blocks_on_an_early_release_filter(slk, nrej):
    s = scenario(8)                                              # the features on clones 1 .. 4: release behind step 8 of 14
    assert release_step(s["feat"][0, :, 3]) == 8 and (s["feat"][:, :, 3] == s["feat"][0, :, 3]).all()
    z = s["z"].copy()
    z[:, 2:4] += 0.8                                             # feature 1 far outside the gate, in every step
    if nrej == 2:
        z[:, 6:8] -= 0.9                                         # and feature 3
    s["z"] = np.ascontiguousarray(z)
    oc = run_and_compare(slk, s, f"{nrej} blocks rejected")
    assert (oc >= STEPS * nrej).all() and (oc < STEPS * 4).all(), oc


# ------------------------------------------------------------------ a covariance that is not positive definite
@pytest.mark.parametrize("row", [2, 35, 50], ids=["before-the-release", "at-the-release-column", "after-the-release"])
def test_first_bad_pivot_around_the_release_column(slk, row):
    """update() factors the covariance as given, inside the update kernel.  A negative diagonal entry at `row` of an otherwise
    SPD matrix: the first pivot that is not positive is that row's.  Row 2 fails before the release, row 35 = jmax in the step
    that releases, row 50 while the other waves are evaluating h(X) on a finished part of the factor."""
    k = 8
    s = scenario(k)
    n, lay = s["P"].shape[0], o.layout(o.MULTI, k)
    assert last_live_column(s["feat"][BAD, :, 3]) == 35
    P = s["P"].copy()
    P[BAD, row, row] = -P[BAD, row, row]
    assert o.cholesky_lower(P[BAD])[1] == row and all(o.cholesky_lower(P[b])[1] == -1 for b in range(n) if b != BAD)
    f = slk.Msckf(s["mean"], P)
    f.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    st, out = f.status(), f.outliers()
    got, Mg = f.getPk(), f.muState()
    r = o.Msckf(k, s["mean"][BAD], P[BAD])
    sto, _ = r.update(s["z"][BAD], o.mm_feature_proj(s["feat"][BAD]), s["R"])
    print(f"first bad pivot at row {row}: status {st}, oracle's {sto}")
    assert sto != 0 and st[BAD] & slk.ST_LLT_FAIL               # the oracle's LLT stops there too
    np.testing.assert_array_equal(got[BAD], P[BAD])              # the state is kept, bit for bit
    np.testing.assert_array_equal(Mg[BAD], s["mean"][BAD])
    for b in range(n):
        if b == BAD:
            continue
        r = o.Msckf(k, s["mean"][b], P[b])
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto == 0 and st[b] & ~slk.ST_ALL_REJECTED == 0 and out[b] == no, b
        assert rel(got[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, b
        np.testing.assert_array_equal(got[b], got[b].T)


# ------------------------------------------------------------------ filters that leave the fast path behind an early h(X)
def test_rotation_column_beyond_the_exponentials_domain(slk):
    """Clone 2's attitude variance grows by 17 rad^2 in one filter: column 22 of its factor is longer than 4 rad in the rows
    that feature 1 (wave 1, released early) moves with -- the exponential of h(X) raises its flag and the rotation bound of
    phase 0 fires as well; the general body computes that filter, the others stay on the fast path."""
    k = 8
    s = scenario(k)
    assert last_live_column(s["feat"][BAD, :, 3]) == 35 and s["feat"][BAD, 1, 3] == 2
    P = s["P"].copy()
    P[BAD, 22, 22] += 17.0
    L = np.linalg.cholesky(P[BAD])
    assert np.linalg.norm(L[21:24, :], axis=0).max() > 4.0
    run_and_compare(slk, s, "rotation column of 4.1 rad on an observed clone", P=np.ascontiguousarray(P),
                    any_rejected_status=True)


@pytest.mark.parametrize("feature", [1, 2, 3])
@pytest.mark.parametrize("index", [9.0, -1.0], ids=["K+1", "minus-one"])
def test_pose_index_out_of_range_on_a_released_wave(slk, feature, index):
    """Device-resident parameters are checked by the kernel: the filter is reported (SLK_ST_BAD_INDEX) and keeps its state, the
    others are updated as in a batch without the bad index.  The wave that evaluates `feature` has run h(X) by then, on the
    clamped index."""
    import torch
    k = 8
    s = scenario(k)
    n = s["P"].shape[0]
    assert last_live_column(s["feat"][BAD, :, 3]) == 35
    feat = s["feat"].copy()
    feat[BAD, feature, 3] = index
    dev = torch.device("cuda", 0)
    d = {name: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for name, v in
         (("feat", feat.reshape(n, -1)), ("z", s["z"]), ("R", s["R"]))}
    f = slk.Msckf(s["mean"], s["P"])
    f.update(d["z"], slk.MM_FEATURE_PROJ, d["feat"], d["R"])
    st = f.status()
    print(f"feature {feature} on pose {index}: status {st}")
    assert st[BAD] == slk.ST_BAD_INDEX and (np.delete(st, BAD) & ~slk.ST_ALL_REJECTED == 0).all()
    np.testing.assert_array_equal(f.getPk()[BAD], s["P"][BAD])
    np.testing.assert_array_equal(f.muState()[BAD], s["mean"][BAD])
    g = slk.Msckf(s["mean"], s["P"])
    g.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    Pf, Pg, Mf, Mg = f.getPk(), g.getPk(), f.muState(), g.muState()
    lay = o.layout(o.MULTI, k)
    for b in range(n):
        if b == BAD:
            continue
        np.testing.assert_array_equal(Pf[b], Pg[b])
        np.testing.assert_array_equal(Mf[b], Mg[b])
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto == 0 and f.outliers()[b] == no and rel(Pf[b], r.P) <= TOL and mean_err(lay, Mf[b], r.mean) <= TOL, b
        np.testing.assert_array_equal(Pf[b], Pf[b].T)
