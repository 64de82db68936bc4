"""The exact-shape Msckf update (k = 4 .. 8, m = 8; csrc/slk_step_fast.hpp) stops four sums at the last column any
measurement row depends on: a feature seen from pose c (0 = the current state, c = clone c) moves only with the sigma columns
j <= tp + 5 (tp = 0, or 6 + 6 c), the lanes beyond evaluate X_0 and their deviations are exact zeros.  With jmax = the
largest tp + 5 of a filter's four features (per workgroup) and ksmax = jmax >> 2 (k-steps of four columns):

  * S = sum y y^T runs the k-steps 0 .. ksmax;
  * the parked block bases of the factor update's prefix sums: slots 0 .. ksmax + 1, every later block reads the last;
  * delta = L b: the groups of eight columns up to the one that holds jmax;
  * L' = L M: below the diagonal the k-steps of a tile M(Kb, J) with 16 Kb + 4 s <= jmax; a diagonal tile keeps all four
    (its rows beyond jmax are identity rows that copy L's columns).

What each bound could lose is checked against the oracle's batch step at the smallest shapes where it can go wrong:

  * k = 8, all four features on one pose c = 0 .. 8: jmax = 5, 17, 23, 29, 35, 41, 47, 53, 59 -- one k-step past a tile edge
    (17), either side of an edge of the groups of eight and of four (29, 35), the last k-step of a tile (47), nothing
    skipped (59);
  * k = 4 (NT = 3, NKS = 9) with c = 0, 2, 4 (jmax = N - 1 at c = 4);
  * mixed poses where the maximum decides ([0, 0, 0, 5], [4, 1, 1, 1]) and a batch whose filters differ in their poses;
  * one and two measurement blocks pushed out of the gate at jmax = 35 (identity rows of M under the k-step skip);
  * for three of the single-pose cases the numpy twin of the oracle (oracle/np_check.py) shows on the host that a wrongly
    dropped live k-step would be seen: S of the first update without its last four live columns moves by far more than
    1e4 TOL relative (asserted of the twin itself; it is 0.54 .. 0.58).
Every case: status == 0, outliers equal to the oracle's, P exactly symmetric.  B = 8 filters, 3 steps; TOL = 1e-9 and the
helpers of tests/test_gpu_routes.py, the scenario builder of tests/test_gpu_matrix_trim.py.  Run with `pytest -m gpu` on an
MI355X.
"""
import numpy as np
import pytest

from oracle import np_check as npc
from oracle import oracle as o
import scenarios as sc
from test_gpu_routes import TOL, colmajor_P, mean_err, rel

pytestmark = pytest.mark.gpu
B, STEPS, M = 8, 3, 8


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def last_live_column(poses):
    """jmax of the kernel: the last column any measurement row depends on (pose c: rows 6 + 6 c .. 11 + 6 c, the current
    state rows 0 .. 5)."""
    return max((6 + 6 * int(c) if c else 0) + 5 for c in poses)


def scenario(k, poses=None, seed_tag=0):
    """The synthetic scenario with the four features observed from the given poses: one list of four for every filter, or
    one list per filter."""
    s = sc.synthetic_msckf(B, k, m=M, seed=0x11CB0000 + k)
    if poses is None:
        return s
    poses = np.broadcast_to(np.asarray(poses, dtype=np.int64), (B, 4))
    rng = np.random.default_rng(0x11CB1000 + 64 * k + seed_tag)
    mean, feat, z = s["mean"], s["feat"].copy(), s["z"].copy()
    for j in range(4):
        c = poses[:, j]
        at = np.where(c == 0, 0, 13 + 7 * (c - 1))
        pos = np.stack([mean[b, at[b]:at[b] + 3] for b in range(B)])
        quat = np.stack([mean[b, at[b] + 3:at[b] + 7] for b in range(B)])
        local = np.concatenate([rng.uniform(-1, 1, (B, 2)), rng.uniform(4, 8, (B, 1))], axis=1)
        feat[:, j, 0:3] = pos + sc.quat_rotate(quat, local)
        feat[:, j, 3] = c
        z[:, 2 * j:2 * j + 2] = local[:, 0:2] / local[:, 2:3] + rng.normal(0, 0.05, (B, 2))
    s["feat"], s["z"] = np.ascontiguousarray(feat), np.ascontiguousarray(z)
    return s


def run_and_compare(slk, s, label):
    k, N, lay, P = s["k"], s["N"], o.layout(o.MULTI, s["k"]), s["P"]
    f = slk.Msckf(s["mean"], P)
    tot = np.zeros(B, dtype=np.int64)
    for _ in range(STEPS):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += f.outliers()
    st = f.status()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(B, -1)
    sto, oc = o.msckf_step_batch(k, M, STEPS, om, oP, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    oP = colmajor_P(oP, N)
    Pg, Mg = f.getPk(), f.muState()
    errs = [(rel(Pg[b], oP[b]), mean_err(lay, Mg[b], om[b])) for b in range(B)]
    print(f"k={k} {label}: status {st}, outliers {tot} / oracle {oc}, worst P {max(e[0] for e in errs):.2e}, "
          f"mean {max(e[1] for e in errs):.2e}")
    assert sto == 0
    assert (st == 0).all()
    np.testing.assert_array_equal(tot, oc)
    for b in range(B):
        assert errs[b][0] <= TOL and errs[b][1] <= TOL, (b, errs[b])
        np.testing.assert_array_equal(Pg[b], Pg[b].T)
    return oc


def s_move_without_last_live_columns(s, b, jmax):
    """max |S - S'| / max |S| of filter b's first update on the numpy twin, S' = S without the terms of the sigma pairs of
    the columns jmax - 3 .. jmax: what a k-step dropped one too early would lose."""
    k, u = s["k"], s["u"][b]
    flt = npc.Msckf(k, s["mean"][b], s["P"][b])
    flt.predict(lambda x: npc.pm_delta_pose(x, u[0:3], u[3:7], u[7:10], u[10:13]), s["Q"])
    X = flt.man.sigma(flt.mean, np.zeros(flt.man.N), flt.P)
    Z = np.array([npc.mm_feature_proj(x, s["feat"][b]) for x in X])
    dZ = Z - Z.sum(axis=0) / len(Z)
    S = 0.5 * dZ.T @ dZ + s["R"]
    beyond = dZ[1 + 2 * (jmax + 1):] - dZ[0]
    assert np.array_equal(beyond, np.zeros_like(beyond))        # the columns beyond jmax: exact zeros about Z_0, on the twin too
    rows = [1 + 2 * j + h for j in range(jmax - 3, jmax + 1) for h in (0, 1)]
    Sd = S - 0.5 * dZ[rows].T @ dZ[rows]
    return float(np.abs(S - Sd).max() / np.abs(S).max())


TWIN_CASES = (1, 4, 7)                                           # jmax = 17, 35, 53


@pytest.mark.parametrize("c", list(range(9)))
def test_k8_all_features_on_one_pose(slk, c):
    poses = [c] * 4
    jmax = last_live_column(poses)
    assert jmax == (5, 17, 23, 29, 35, 41, 47, 53, 59)[c]
    s = scenario(8, poses)
    if c in TWIN_CASES:
        move = [s_move_without_last_live_columns(s, b, jmax) for b in (0, 5)]
        print(f"k=8 pose {c}: S without the columns {jmax - 3} .. {jmax} moves by {move} (numpy twin)")
        assert min(move) > 1e4 * TOL, move
    run_and_compare(slk, s, f"poses {poses} (jmax = {jmax})")


@pytest.mark.parametrize("c", [0, 2, 4])
def test_k4_all_features_on_one_pose(slk, c):
    poses = [c] * 4
    jmax = last_live_column(poses)
    assert jmax == {0: 5, 2: 23, 4: 35}[c] and (c != 4 or jmax == 12 + 6 * 4 - 1)
    run_and_compare(slk, scenario(4, poses), f"poses {poses} (jmax = {jmax})")


@pytest.mark.parametrize("poses,jmax", [([0, 0, 0, 5], 41), ([4, 1, 1, 1], 35)])
def test_mixed_poses_the_maximum_decides(slk, poses, jmax):
    assert last_live_column(poses) == jmax
    run_and_compare(slk, scenario(8, poses, seed_tag=1 + poses[0]), f"poses {poses} (jmax = {jmax})")


def test_filters_of_one_batch_differ_in_their_poses(slk):
    poses = [[0, 0, 0, 0], [1, 1, 1, 1], [4, 1, 1, 1], [0, 0, 0, 5], [8, 8, 8, 8], [2, 7, 2, 2], [3, 3, 3, 3], [6, 0, 6, 0]]
    assert [last_live_column(p) for p in poses] == [5, 17, 35, 41, 59, 53, 29, 47]
    run_and_compare(slk, scenario(8, poses, seed_tag=9), "poses per filter")


@pytest.mark.parametrize("nrej", [1, 2])
def test_rejected_blocks_at_jmax_35(slk, nrej):
    s = scenario(8)                                              # the features on clones 1 .. 4
    assert last_live_column(s["feat"][0, :, 3]) == 35 and (s["feat"][:, :, 3] == s["feat"][0, :, 3]).all()
    z = s["z"].copy()
    z[:, 2:4] += 0.8                                             # feature 1 far outside the gate, in every step
    if nrej == 2:
        z[:, 6:8] -= 0.9                                         # and feature 3
    s["z"] = np.ascontiguousarray(z)
    oc = run_and_compare(slk, s, f"{nrej} blocks rejected")
    assert (oc >= STEPS * nrej).all() and (oc < STEPS * 4).all(), oc
