"""The exact-shape Msckf update (k = 4 .. 8, m = 8; csrc/slk_step_fast.hpp) releases the first factorisation's finished columns
more than once (csrc/slk_math.hpp: fast_release_plan).  With r_f = (tp_f + 5) >> 2 the step that leaves feature f's rows final and
e0 .. e3 the features ordered by (r_f, f): where r_e1 + 3 <= ksmax = r_e3 and C = ksmax + 3 <= NKS - 2 wave 0 meets the other
waves behind step A = r_e1 (the waves 1 and 2 evaluate e0 and e1 while it factors on), behind step B = ksmax (e2 and e3) and
behind step C (S on wave 1 and the prefix sums on wave 3, under the last steps; the barrier that closes h(X) is then the one
behind S as well).  Otherwise the single release at ksmax -- also where A and B would fit but C would not: A + B alone measured
behind the single release.  No operation changes, so every case is the oracle's batch step:

  * the k = 8 tuples of the table: [1,2,3,4] (5 / 8 / 11), [0,0,0,5] (1 / 10 / 13), [0,1,8,8] (A and B would stand at 4 / 14, no
    room for C: single release), the single-release tuples [3,3,3,4], [4,4,4,4], [8,8,8,8], [0,0,0,0], and the permutations
    [4,3,2,1] and [2,4,1,3]: the assignment follows the order of release, not the feature index;
  * the tie [1,1,4,4];
  * k = 7 [1,2,4,4], k = 6 [0,1,3,3], k = 5 [0,0,2,2] (staggered) and [0,0,3,3], k = 4 [1,2,3,4] (no room for C: single release);
  * a batch whose eight filters have eight different plans, staggered and single-release side by side; batches of 1 and 7;
  * the gate: one and two blocks pushed out on a staggered filter;
  * a covariance whose first bad pivot lies before A, between A and B, between B and C and behind C (rows 2, 30, 40, 50 with
    A / B / C behind the columns 23 / 35 / 47): SLK_ST_LLT_FAIL, the state kept bit for bit, the neighbours in parity;
  * a rotation column beyond 4 rad on a clone that an early-group feature observes;
  * a pose index of K + 1 and of -1 in device-resident parameters, on a feature of each group.
Every case: status, outliers, mean and P against the oracle, P exactly symmetric.  B = 8 filters, 3 steps; TOL = 1e-9 and the
helpers of tests/test_gpu_routes.py, the scenario builder of tests/test_gpu_live_column_bound.py, the comparison of
tests/test_gpu_early_hx.py.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
from test_gpu_early_hx import first_filters, run_and_compare
from test_gpu_live_column_bound import scenario
from test_gpu_routes import TOL, mean_err, rel

pytestmark = pytest.mark.gpu
BAD = 2                                                          # the filter of a batch that is damaged
HS, HC = 3, 3                                                    # one h(X) = three late steps of the factorisation; C = B + HC


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def plan(poses, k=8):
    """(A, B) of the staggered plan, or (None, ksmax) where the single release stands."""
    r = sorted(((6 + 6 * int(c) if c else 0) + 5) >> 2 for c in poses)
    nks = (12 + 6 * k + 3) // 4
    return (r[1], r[3]) if r[1] + HS <= r[3] and r[3] + HC <= nks - 2 else (None, r[3])


# ------------------------------------------------------------------ the plans of the table, k = 8
@pytest.mark.parametrize("poses,ab", [([1, 2, 3, 4], (5, 8)), ([0, 0, 0, 5], (1, 10)), ([0, 1, 8, 8], (None, 14)),
                                      ([3, 3, 3, 4], (None, 8)), ([4, 4, 4, 4], (None, 8)), ([8, 8, 8, 8], (None, 14)),
                                      ([0, 0, 0, 0], (None, 1)), ([4, 3, 2, 1], (5, 8)), ([2, 4, 1, 3], (5, 8)),
                                      ([1, 1, 4, 4], (4, 8))], ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else None)
def test_k8_plans(slk, poses, ab):
    assert plan(poses) == ab
    run_and_compare(slk, scenario(8, poses, seed_tag=3), f"poses {poses} (A, B = {ab})")


@pytest.mark.parametrize("k,poses,ab", [(7, [1, 2, 4, 4], (5, 8)), (6, [0, 1, 3, 3], (4, 7)), (5, [0, 0, 2, 2], (1, 5)),
                                        (5, [0, 0, 3, 3], (None, 7)), (4, [1, 2, 3, 4], (None, 8))],
                         ids=["k7", "k6", "k5-with-C", "k5-without-C", "k4"])
def test_other_instantiations(slk, k, poses, ab):
    assert plan(poses, k) == ab
    run_and_compare(slk, scenario(k, poses, seed_tag=3), f"poses {poses} (A, B = {ab})")


# ------------------------------------------------------------------ filters of one batch on different plans
PER_FILTER = [[1, 2, 3, 4], [0, 0, 0, 5], [0, 1, 8, 8], [3, 3, 3, 4], [2, 0, 7, 6], [0, 0, 0, 0], [1, 1, 4, 4], [0, 3, 5, 5]]


def test_eight_plans_in_one_batch(slk):
    plans = [plan(p) for p in PER_FILTER]
    assert plans == [(5, 8), (1, 10), (None, 14), (None, 8), (None, 13), (None, 1), (4, 8), (7, 10)] and len(set(plans)) == 8
    run_and_compare(slk, scenario(8, PER_FILTER, seed_tag=11), "plans per filter")


@pytest.mark.parametrize("n", [1, 7])
def test_small_batches(slk, n):
    run_and_compare(slk, first_filters(scenario(8, PER_FILTER, seed_tag=11), n), "plans per filter")


# ------------------------------------------------------------------ the gate on a staggered filter
@pytest.mark.parametrize("nrej", [1, 2])
def test_rejected_blocks_on_a_staggered_filter(slk, nrej):
    s = scenario(8)                                              # the features on clones 1 .. 4
    assert plan(s["feat"][0, :, 3]) == (5, 8) and (s["feat"][:, :, 3] == s["feat"][0, :, 3]).all()
    z = s["z"].copy()
    z[:, 0:2] += 0.8                                             # feature 0 (early group) far outside the gate, in every step
    if nrej == 2:
        z[:, 6:8] -= 0.9                                         # and feature 3 (late group)
    s["z"] = np.ascontiguousarray(z)
    oc = run_and_compare(slk, s, f"{nrej} blocks rejected")
    assert (oc >= 3 * nrej).all() and (oc < 3 * 4).all(), oc


# ------------------------------------------------------------------ a covariance that is not positive definite
@pytest.mark.parametrize("row", [2, 30, 40, 50], ids=["before-A", "between-A-and-B", "between-B-and-C", "behind-C"])
def test_first_bad_pivot_around_the_releases(slk, row):
    """A negative diagonal entry at `row` of an otherwise SPD matrix: the first pivot that is not positive is that row's.  With
    the features on the clones 1 .. 4 the releases stand behind the steps 5, 8 and 11 (columns 23, 35, 47): row 2
    fails before any wave is released, row 30 while the early pair is evaluated, row 40 while the late pair is, row 50 beside S
    and the prefix sums -- all of them on a factor that is about to be thrown away."""
    k = 8
    s = scenario(k)
    n, lay = s["P"].shape[0], o.layout(o.MULTI, k)
    assert plan(s["feat"][BAD, :, 3]) == (5, 8)
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
def test_rotation_column_beyond_the_exponentials_domain_in_the_early_group(slk):
    """Clone 1's attitude variance grows by 17 rad^2 in one filter: column 16 of its factor is longer than 4 rad in the rows that
    feature 0 (early group, evaluated behind A) moves with -- the exponential of h(X) raises its flag under the factorisation
    and the rotation bound of phase 0 fires as well; the general body computes that filter, the others stay on the fast path."""
    k = 8
    s = scenario(k)
    assert plan(s["feat"][BAD, :, 3]) == (5, 8) and s["feat"][BAD, 0, 3] == 1
    P = s["P"].copy()
    P[BAD, 16, 16] += 17.0
    L = np.linalg.cholesky(P[BAD])
    assert np.linalg.norm(L[15:18, :], axis=0).max() > 4.0
    run_and_compare(slk, s, "rotation column of 4.1 rad on a clone of the early group", P=np.ascontiguousarray(P),
                    any_rejected_status=True)


@pytest.mark.parametrize("feature", [0, 3], ids=["early-group", "late-group"])
@pytest.mark.parametrize("index", [9.0, -1.0], ids=["K+1", "minus-one"])
def test_pose_index_out_of_range(slk, feature, index):
    """Device-resident parameters are checked by the kernel: the filter is reported (SLK_ST_BAD_INDEX) and keeps its state, the
    others are updated as in a batch without the bad index.  The plan is made from the clamped indices, the same ones h(X)
    forms its addresses from."""
    import torch
    k = 8
    s = scenario(k)
    n = s["P"].shape[0]
    assert plan(s["feat"][BAD, :, 3]) == (5, 8)
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
