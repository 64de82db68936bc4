"""The first factorisation inside the fast-path update kernels (csrc/slk_kernels.hpp, CholPSteps / cholp_factor) skips what the
result does not need: steps whose four columns are all padding only store the zeros of the tile layout, the padding columns
of a partially live step are neither pivoted nor tested, and the last live step forms no fragment and no trailing update.
What that trimming can lose is checked here, for every padding case of the fast path (N = 12 + 6 k, tiles of 16):

  k   N   first partial step   steps that are all padding
  4   36  --                   k0 = 36, 40, 44 (the third tile row has 4 live rows)
  5   42  k0 = 40 (2 live)     k0 = 44
  6   48  --                   -- (the third tile row is exactly full)
  7   54  k0 = 52 (2 live)     k0 = 56, 60
  8   60  --                   k0 = 60

  * parity of the fused step with the oracle per shape;
  * a covariance whose LAST live pivot is the only one that is not positive (positive diagonal, Schur complement of column
    N - 1 below zero): reported, state kept, the healthy neighbours untouched and in parity -- so neither is the last pivot
    test lost nor does a padding "pivot" raise the flag;
  * the Usckf unit shape (N = 48, m = 3), whose update kernel runs the same factor code.
Tolerance: TOL = 1e-9 as tests/test_gpu_routes.py holds the same routes to ("k8-m8-exact", "k5-m8-exact", "usckf-unit-fast").
Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
from test_gpu_routes import TOL, colmajor_P, mean_err, pm_dp, rel

pytestmark = pytest.mark.gpu
M = 8


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


@pytest.mark.parametrize("k", [4, 5, 6, 7, 8])
def test_fast_path_step_parity_per_padding_case(slk, k):
    B, steps = 3, 3
    s = sc.synthetic_msckf(B, k, m=M, seed=0x5EEDFA00 + k)
    N, lay = s["N"], o.layout(o.MULTI, k)
    f = slk.Msckf(s["mean"], s["P"])
    tot = np.zeros(B, dtype=np.int64)
    for _ in range(steps):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += f.outliers()
    assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    st, oc = o.msckf_step_batch(k, M, steps, om, oP, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    assert st == 0
    oP = colmajor_P(oP, N)
    P, Mg = f.getPk(), f.muState()
    worst_P = max(rel(P[b], oP[b]) for b in range(B))
    worst_m = max(mean_err(lay, Mg[b], om[b]) for b in range(B))
    print(f"k={k} N={N}: P {worst_P:.2e} mean {worst_m:.2e} outliers {tot} / {oc}")
    np.testing.assert_array_equal(tot, oc)
    assert worst_P <= TOL and worst_m <= TOL


def _schur_last(P):
    """The Schur complement of the last column: the pivot an exact LLT meets there."""
    w = P[:-1, -1]
    return float(P[-1, -1] - w @ np.linalg.solve(P[:-1, :-1], w))


def _fails_at_last_only(P):
    N = P.shape[0]
    return o.cholesky_lower(P)[1] == N - 1 and o.cholesky_lower(P[:N - 1, :N - 1])[1] == -1


@pytest.mark.parametrize("k", [7, 8])
def test_last_live_pivot_not_positive_update(slk, k):
    """update(): the covariance is factored as given.  Filter 1's P[N-1, N-1] is lowered until the Schur complement of the
    last column is -0.1 % of what it was: the diagonal stays positive, every leading block stays SPD."""
    s = sc.synthetic_msckf(3, k, m=M, seed=0x5EEDFB00 + k)
    N, lay = s["N"], o.layout(o.MULTI, k)
    P = s["P"].copy()
    sch = _schur_last(P[1])
    P[1, N - 1, N - 1] -= 1.001 * sch
    assert P[1, N - 1, N - 1] > 0 and _fails_at_last_only(P[1])
    assert all(o.cholesky_lower(P[b])[1] == -1 for b in (0, 2))
    f = slk.Msckf(s["mean"], P)
    f.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    st = f.status()
    print(f"k={k}: Schur complement {sch:.3e} -> {_schur_last(P[1]):.3e}, status {st}")
    assert list(st) == [0, slk.ST_LLT_FAIL, 0]
    got, Mg = f.getPk(), f.muState()
    np.testing.assert_array_equal(got[1], P[1])
    np.testing.assert_array_equal(Mg[1], s["mean"][1])
    out = f.outliers()
    for b in (0, 2):                               # the healthy neighbours: no flag from a padding column, oracle parity
        r = o.Msckf(k, s["mean"][b], P[b])
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto == 0 and out[b] == no
        assert rel(got[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL


@pytest.mark.parametrize("k", [7, 8])
def test_last_live_pivot_not_positive_step(slk, k):
    """step(): the update factors the PREDICTED covariance.  The prediction leaves P[N-1, N-1] (the last clone's block) as it
    is, so that entry is lowered by the predicted matrix's Schur complement; the oracle's prediction confirms where its LLT
    fails.  The failing filter keeps its predicted state (what predict() alone leaves), the neighbours match the oracle."""
    s = sc.synthetic_msckf(3, k, m=M, seed=0x5EEDFC00 + k)
    N, lay = s["N"], o.layout(o.MULTI, k)

    def predicted(P1):
        r = o.Msckf(k, s["mean"][1], P1)
        assert r.predict(pm_dp(s["u"][1]), s["Q"]) == 0
        return r.P

    P = s["P"].copy()
    P[1, N - 1, N - 1] -= 1.001 * _schur_last(predicted(P[1]))
    Pp = predicted(P[1])
    assert P[1, N - 1, N - 1] > 0 and Pp[N - 1, N - 1] == P[1, N - 1, N - 1] and _fails_at_last_only(Pp)
    f, g = slk.Msckf(s["mean"], P), slk.Msckf(s["mean"], P)
    f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    g.predict(slk.PM_DELTA_POSE, s["u"], s["Q"])
    st = f.status()
    print(f"k={k}: predicted Schur complement {_schur_last(Pp):.3e}, status {st}")
    assert list(st) == [0, slk.ST_LLT_FAIL, 0]
    assert (g.status() == 0).all()
    got, Mg = f.getPk(), f.muState()
    np.testing.assert_array_equal(got[1], g.getPk()[1])
    np.testing.assert_array_equal(Mg[1], g.muState()[1])
    assert rel(got[1], Pp) <= TOL
    om = s["mean"][[0, 2]].copy()
    oP = np.ascontiguousarray(np.transpose(P[[0, 2]], (0, 2, 1))).reshape(2, -1)
    sto, oc = o.msckf_step_batch(k, M, 1, om, oP, s["u"][[0, 2]].copy(), s["feat"][[0, 2]].copy(), s["z"][[0, 2]].copy(),
                                 s["Q"], s["R"])
    assert sto == 0
    oP = colmajor_P(oP, N)
    np.testing.assert_array_equal(f.outliers()[[0, 2]], oc)
    for j, b in enumerate((0, 2)):
        assert rel(got[b], oP[j]) <= TOL and mean_err(lay, Mg[b], om[j]) <= TOL


def test_usckf_unit_shape_parity(slk):
    """N = 48 = three full tile rows: no padding step, but the last step's trimming and the retired tile columns apply."""
    B, nfk, nfkl, steps = 3, 3, 9, 3
    s = sc.synthetic_usckf(B, seed=0x5EEDFD00)
    N, lay = s["N"], o.layout(o.AUGMENTED, 0, nfk, nfkl)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    for _ in range(steps):
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    assert o.usckf_step_batch(nfk, nfkl, steps, om, oP, s["u"], s["z"], s["Q"], s["R"]) == 0
    oP = colmajor_P(oP, N)
    P, Mg = f.PkAugmentedState(), f.muState()
    for b in range(B):
        assert rel(P[b], oP[b]) <= TOL and mean_err(lay, Mg[b], om[b]) <= TOL
