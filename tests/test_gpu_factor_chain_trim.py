"""The one-wave chains of the fast-path update kernels carry their pivot test on the scalar side (csrc/slk_math.hpp:
pivot_rank_neg), keep the panel's sign folded into the scale, store the factor's columns under lane masks into zero-filled tiles
and set the gain phase up without selects when every row survives the gate (csrc/slk_kernels.hpp: CholPSteps,
csrc/slk_step_fast.hpp).  None of that changes a number; what it could lose is checked here:

  * a pivot test that is lost, or fires a column early or late: covariances L D L^T with D = I except -eps at column j, j at
    each of the four positions of a panel step in mid-matrix (j = 20 .. 23), for the exact shapes k = 5 (N = 42, partial
    step k0 = 40) and k = 8 (N = 60) -- reported, state kept, the healthy neighbours of the batch in parity with the oracle;
  * a NaN on a mid-matrix diagonal, and a pivot that is exactly zero (row and column j all zero);
  * the same mid-panel case through the stand-alone factor kernel (k = 8, m = 4: three launches) and the Usckf unit shape
    (N = 48, m = 3), which run the same panel step with the packed outputs;
  * the gate: at k = 4 and k = 8 one batch in which no block is rejected (kept == 0xff), one block of one filter is, and three
    of four of another are -- state and outliers against the oracle, the plain and the masked set-up in the same launch.
B = 6 filters, 3 steps; helpers and TOL = 1e-9 of tests/test_gpu_routes.py.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
from test_gpu_routes import TOL, colmajor_P, mean_err, pm_cv, ref_usckf, rel

pytestmark = pytest.mark.gpu
B, STEPS, EPS = 6, 3, 1e-3
BAD = 2                                        # the filter of the batch whose covariance is damaged


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def ldl_with_negative_pivot(P, j, eps=EPS):
    """L D L^T of P's own factor with D = I except D[j, j] = -eps: an exact LLT meets pivot j = -eps L[j, j]^2, every pivot
    before it is the positive one of P."""
    L = np.linalg.cholesky(P)
    D = np.ones(P.shape[0])
    D[j] = -eps
    Q = (L * D) @ L.T
    return 0.5 * (Q + Q.T)


def damaged(P, how, j):
    P = P.copy()
    if how == "negative":
        P[BAD] = ldl_with_negative_pivot(P[BAD], j)
    elif how == "nan":
        P[BAD, j, j] = np.nan
    else:                                      # "zero": the pivot is exactly 0 (nothing is subtracted from a zero diagonal)
        P[BAD, j, :] = 0.0
        P[BAD, :, j] = 0.0
    return P


def fails_at(P, j):
    """Where the oracle's LLT stops: column j (a NaN pivot is not positive either), with every leading block SPD."""
    return o.cholesky_lower(P)[1] == j and o.cholesky_lower(P[:j, :j])[1] == -1


CASES = [("negative", j) for j in (20, 21, 22, 23)] + [("nan", 21), ("zero", 22)]


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("how,j", CASES, ids=[f"{h}-{j}" for h, j in CASES])
def test_mid_panel_pivot_update(slk, k, how, j):
    """update() factors the covariance as given (exact shapes: inside the update kernel, wave 0)."""
    m = 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0x5EEDCA00 + k)
    N, lay = s["N"], o.layout(o.MULTI, k)
    P = damaged(s["P"], how, j)
    assert fails_at(P[BAD], j) and all(o.cholesky_lower(P[b])[1] == -1 for b in range(B) if b != BAD)
    if how == "negative":
        assert P[BAD, j, j] > 0                # (only the factorisation can tell)
    f = slk.Msckf(s["mean"], P)
    f.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    st, out = f.status(), f.outliers()
    got, Mg = f.getPk(), f.muState()
    print(f"k={k} {how} j={j}: status {st}")
    assert st[BAD] & slk.ST_LLT_FAIL
    np.testing.assert_array_equal(got[BAD], P[BAD])                  # (NaN == NaN position-wise)
    np.testing.assert_array_equal(Mg[BAD], s["mean"][BAD])
    for b in range(B):
        if b == BAD:
            continue
        r = o.Msckf(k, s["mean"][b], P[b])
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto == 0 and st[b] & ~slk.ST_ALL_REJECTED == 0 and out[b] == no, b
        assert rel(got[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, b


@pytest.mark.parametrize("k", [5, 8])
def test_healthy_batch_three_steps(slk, k):
    """No pivot test fires where none should: three fused steps of the undamaged batch against the oracle."""
    m = 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0x5EEDCA00 + k)
    N, lay = s["N"], o.layout(o.MULTI, k)
    f = slk.Msckf(s["mean"], s["P"])
    tot = np.zeros(B, dtype=np.int64)
    for _ in range(STEPS):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += f.outliers()
    assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    sto, oc = o.msckf_step_batch(k, m, STEPS, om, oP, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    assert sto == 0
    oP = colmajor_P(oP, N)
    P, Mg = f.getPk(), f.muState()
    np.testing.assert_array_equal(tot, oc)
    for b in range(B):
        assert rel(P[b], oP[b]) <= TOL and mean_err(lay, Mg[b], om[b]) <= TOL, b


def test_mid_panel_pivot_factor_kernel(slk):
    """k = 8 with m = 4 rows leaves the exact-shape kernel: the factor comes from the stand-alone factor kernel (packed,
    through the workspace), three launches per step."""
    k, m, j = 8, 4, 21
    s = sc.synthetic_msckf(B, k, m=m, seed=0x5EEDCB00)
    N, lay = s["N"], o.layout(o.MULTI, k)
    P = damaged(s["P"], "negative", j)
    assert fails_at(P[BAD], j)
    f = slk.Msckf(s["mean"], P)
    f.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    st, out = f.status(), f.outliers()
    got, Mg = f.getPk(), f.muState()
    assert st[BAD] & slk.ST_LLT_FAIL
    np.testing.assert_array_equal(got[BAD], P[BAD])
    np.testing.assert_array_equal(Mg[BAD], s["mean"][BAD])
    for b in range(B):
        if b == BAD:
            continue
        r = o.Msckf(k, s["mean"][b], P[b])
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto == 0 and st[b] & ~slk.ST_ALL_REJECTED == 0 and out[b] == no, b
        assert rel(got[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, b
    # and three fused steps of the healthy batch on the same route
    g = slk.Msckf(s["mean"], s["P"])
    tot = np.zeros(B, dtype=np.int64)
    for _ in range(STEPS):
        g.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += g.outliers()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    sto, oc = o.msckf_step_batch(k, m, STEPS, om, oP, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    assert sto == 0 and (g.status() & ~slk.ST_ALL_REJECTED == 0).all()
    oP = colmajor_P(oP, N)
    np.testing.assert_array_equal(tot, oc)
    Pg, Mg = g.getPk(), g.muState()
    for b in range(B):
        assert rel(Pg[b], oP[b]) <= TOL and mean_err(lay, Mg[b], om[b]) <= TOL, b


def test_mid_panel_pivot_usckf_unit_shape(slk):
    """N = 48, m = 3: the Usckf update kernel runs the same panel step into the packed factor in LDS."""
    nfk, nfkl, j = 3, 9, 22
    s = sc.synthetic_usckf(B, seed=0x5EEDCC00)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    P = damaged(s["P"], "negative", j)
    assert fails_at(P[BAD], j)
    f = slk.Usckf(mean=s["mean"], P=P, nfk=nfk, nfkl=nfkl)
    f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    st = f.status()
    got, Mg = f.PkAugmentedState(), f.muState()
    assert st[BAD] & slk.ST_LLT_FAIL
    np.testing.assert_array_equal(got[BAD], P[BAD])
    np.testing.assert_array_equal(Mg[BAD], s["mean"][BAD])
    for b in range(B):
        if b == BAD:
            continue
        r = ref_usckf(s, b, nfk, nfkl, P=P[b])
        sto, acc = r.update(s["z"][b], o.mm_vo_relative(), s["R"])
        assert sto == 0 and acc == 1 and st[b] == 0, b
        assert rel(got[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, b
    # three fused steps of the healthy batch
    g = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    for _ in range(STEPS):
        g.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (g.status() == 0).all()
    Pg, Mg = g.PkAugmentedState(), g.muState()
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        for _ in range(STEPS):
            assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
            assert r.update(s["z"][b], o.mm_vo_relative(), s["R"]) == (0, 1)
        assert rel(Pg[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, b


# filter -> the features (blocks of two rows) whose innovation is moved far out
GATE_CASES = {"none": {}, "one-block": {1: (3,)}, "three-of-four": {1: (3,), 4: (1, 2, 3)}}


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("case", list(GATE_CASES), ids=list(GATE_CASES))
def test_gate_plain_and_masked_setup(slk, k, case):
    """The gain phase's set-up is specialised on kept == 0xff: filters with and without rejected blocks share a launch."""
    m = 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0x5EEDCD00 + k, meas_sigma=0.01)
    N, lay = s["N"], o.layout(o.MULTI, k)
    z = s["z"].copy()
    want = np.zeros(B, dtype=np.int64)
    for b, feats in GATE_CASES[case].items():
        for ft in feats:
            z[b, 2 * ft:2 * ft + 2] += 3.0     # thirty standard deviations of R
        want[b] = len(feats)
    f = slk.Msckf(s["mean"], s["P"])
    first, tot = None, np.zeros(B, dtype=np.int64)
    for _ in range(STEPS):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], z, slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += f.outliers()
        first = f.outliers().copy() if first is None else first
    st = f.status()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    o1m, o1P = om.copy(), oP.copy()
    sto1, oc1 = o.msckf_step_batch(k, m, 1, o1m, o1P, s["u"], s["feat"], z, s["Q"], s["R"])
    sto, oc = o.msckf_step_batch(k, m, STEPS, om, oP, s["u"], s["feat"], z, s["Q"], s["R"])
    assert sto1 == 0 and sto == 0
    np.testing.assert_array_equal(oc1, want)   # the case is what it says: exactly these blocks leave in the first step
    print(f"k={k} {case}: outliers first step {first}, total {tot} / oracle {oc}, status {st}")
    np.testing.assert_array_equal(first, oc1)
    np.testing.assert_array_equal(tot, oc)
    assert (st & ~slk.ST_ALL_REJECTED == 0).all()
    oP = colmajor_P(oP, N)
    P, Mg = f.getPk(), f.muState()
    for b in range(B):
        assert rel(P[b], oP[b]) <= TOL and mean_err(lay, Mg[b], om[b]) <= TOL, b
