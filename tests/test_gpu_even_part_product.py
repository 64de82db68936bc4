"""The exact-shape Msckf update (k = 4 .. 8, m = 8) forms the even-part product E^ E^^T of the covariance rebuild in the index
space of the rotation rows and adds it where the tiles of P+ leave for memory (csrc/slk_step_fast.hpp).  This module runs that
path where the product is not negligible -- the synthetic scenario after 25 steps, when the rotation variance of the current
state has grown by Q every step -- and checks one further step from the state read back at that point against

  * the fp64 CPU oracle, at the tolerance of tests/test_gpu_parity.py for the same quantities;
  * the general body of the same instantiation (slk_update_selected with every row kept: the fast path bails on gate 2),
    which knows nothing of E^, on the vector-row x vector-row entries of P+ and on the whole matrix;
  * exact symmetry of the 16 x 16 diagonal tiles, which the store writes whole from one accumulator orientation.

Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
import test_gpu_parity as parity
import test_gpu_caller_gate as cg

pytestmark = pytest.mark.gpu
TOL = parity.TOL
rel, mean_err = parity.rel, parity.mean_err
WARM = 25


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def rotation_rows(k):
    """Tangent rows of the SO(3) blocks: 3 .. 5 of the current state, 15 + 6 c .. 17 + 6 c of clone c."""
    return np.array([3, 4, 5] + [15 + 6 * c + r for c in range(k) for r in range(3)])


@pytest.mark.parametrize("k", [4, 5, 6, 7, 8])
def test_even_part_product_in_the_rotation_row_space(slk, k):
    B, m = 8, 8
    s = sc.synthetic_msckf(B, k, m=m, seed=4100 + k)
    lay = o.layout(o.MULTI, k)
    N = s["N"]
    step = lambda f: f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])   # noqa: E731
    warm = slk.Msckf(s["mean"], s["P"])
    for _ in range(WARM):
        step(warm)
    assert (warm.status() & ~slk.ST_ALL_REJECTED == 0).all()
    M0, P0 = warm.muState(), warm.getPk()
    # the regime: the current state's rotation variance has grown by Q = 0.01 per axis and step, deviations of a fraction
    # of a radian, whose even parts are of second order in them -- many orders above the tolerance
    rot_var = np.array([np.trace(P0[b][3:6, 3:6]) for b in range(B)])
    print(f"k={k}: rotation variance of the current state after {WARM} steps: min {rot_var.min():.3f} max {rot_var.max():.3f} rad^2")
    assert rot_var.min() > 0.1

    fast = slk.Msckf(M0, P0)
    step(fast)
    gen = slk.Msckf(M0, P0)
    gen.predict(slk.PM_DELTA_POSE, s["u"], s["Q"])
    rsel = cg.make_rowsel([list(range(m))] * B, [0] * B, m)
    assert cg.selected(slk, gen, slk.MM_FEATURE_PROJ, s["feat"], s["z"], s["R"], rsel) == 0
    mean, P = M0.copy(), P0.copy()
    st, out = o.msckf_step_batch(k, m, 1, mean, P, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    assert st == 0
    assert (fast.status() == 0).all() and (gen.status() == 0).all()
    # nothing gated out: the three computations use the same eight rows
    np.testing.assert_array_equal(out, 0)
    np.testing.assert_array_equal(fast.outliers(), 0)

    Pf, Mf = fast.getPk(), fast.muState()
    Pg, Mg = gen.getPk(), gen.muState()
    rot = rotation_rows(k)
    vec = np.setdiff1d(np.arange(N), rot)
    worst = dict(P=0.0, mean=0.0, Pgen=0.0, vec=0.0, meangen=0.0)
    for b in range(B):
        Po = P[b].reshape(N, N).T
        worst["P"] = max(worst["P"], rel(Pf[b], Po))
        worst["mean"] = max(worst["mean"], mean_err(lay, Mf[b], mean[b]))
        worst["Pgen"] = max(worst["Pgen"], rel(Pf[b], Pg[b]))
        worst["vec"] = max(worst["vec"], float(np.abs(Pf[b][np.ix_(vec, vec)] - Pg[b][np.ix_(vec, vec)]).max() / np.abs(Pg[b]).max()))
        worst["meangen"] = max(worst["meangen"], mean_err(lay, Mf[b], Mg[b]))
    print(f"k={k}: fast path against the oracle: P {worst['P']:.2e} mean {worst['mean']:.2e}; against the general body: "
          f"P {worst['Pgen']:.2e} (vector x vector entries {worst['vec']:.2e}) mean {worst['meangen']:.2e}")
    for b in range(B):
        Po = P[b].reshape(N, N).T
        assert rel(Pf[b], Po) <= TOL, b
        assert mean_err(lay, Mf[b], mean[b]) <= TOL, b
        # the general body on the same inputs: the entries E^ does not reach, then everything
        assert np.abs(Pf[b][np.ix_(vec, vec)] - Pg[b][np.ix_(vec, vec)]).max() / np.abs(Pg[b]).max() <= TOL, b
        assert rel(Pf[b], Pg[b]) <= TOL and mean_err(lay, Mf[b], Mg[b]) <= TOL, b
        for t in range(0, N, 16):
            d = Pf[b][t:t + 16, t:t + 16]
            np.testing.assert_array_equal(d, d.T, err_msg=f"filter {b}, diagonal tile at {t}")
        np.testing.assert_array_equal(Pf[b], Pf[b].T)
