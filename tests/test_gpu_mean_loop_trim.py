"""The manifold-mean loop of the exact-shape Msckf update (csrc/slk_step_fast.hpp) stops on the squared norm of mean_delta,
summed where mean_delta is formed (one partial sum per wave, csrc/slk_math.hpp: MEAN_STOP_SQ), and its exp / log series take
the direct or the angle-halving form behind wave-uniform branches, with the domain tests folded over a call's arguments.  None
of that changes a number that reaches the outputs; what it could lose is checked here, against the oracle's batch step:

  * k = 4 (NP = 114 pairs: only waves 0 and 1 hold pairs, wave 3 has no rotation row and contributes a zero partial sum),
    k = 7 (NP = 258: two leftover pairs in wave 1's second round) and k = 8 (NP = 318, the benchmark's shape);
  * small rotations: the rotation blocks of P scaled down, every wave on the direct series;
  * mixed waves: a rotation column of 1.4 rad in the current state of one filter, of 1.2 rad in the newest clone of another --
    waves of one workgroup take different branches;
  * beyond the series: a rotation column of 4.1 rad (beyond 4 rad, and beyond pi): the general body's case, its neighbours in
    the batch unaffected;
  * different pass counts in one launch: a covariance scaled down until the first mean_delta is below 1e-6 (one pass), the
    synthetic scale (two), rotation deviations of 1 rad in every block and a larger innovation (three) -- the counts are those of the numpy twin
    of the oracle (oracle/np_check.py) for the first step and are asserted of IT, not of the kernel.
B = 6 filters, 3 steps; TOL = 1e-9 and the helpers of tests/test_gpu_routes.py.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import np_check as npc
from oracle import oracle as o
import scenarios as sc
from test_gpu_routes import TOL, colmajor_P, mean_err, rel

pytestmark = pytest.mark.gpu
B, STEPS, M = 6, 3, 8
SHAPES = [4, 7, 8]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def rot_rows(k, block):
    """Tangent rows of SO(3) block `block`: 0 = the current state's attitude, c = clone c's."""
    t = 3 if block == 0 else 9 + 6 * block
    return [t, t + 1, t + 2]


def all_rot_rows(k):
    return [t for b in range(k + 1) for t in rot_rows(k, b)]


def scenario(k):
    return sc.synthetic_msckf(B, k, m=M, seed=0x5EEDCE00 + k)


def small_rotations(k):
    """Rotation rows and columns of P scaled by 1/4 (a congruence: P stays SPD): rotation columns of ~0.03 rad."""
    s = scenario(k)
    d = np.ones(s["N"])
    d[all_rot_rows(k)] = 0.25
    return s, np.ascontiguousarray(s["P"] * d[None, :, None] * d[None, None, :])


def mixed_waves(k):
    """As tests/test_gpu_parity.py builds its columns beyond one radian: variance added on a rotation diagonal."""
    s = scenario(k)
    P = s["P"].copy()
    P[1, 3, 3] += 2.0                                            # current state, 1.4 rad: the first pair lanes (wave 0)
    t = rot_rows(k, k)[1]
    P[4, t, t] += 1.5                                            # newest clone, 1.2 rad: the last pair lanes
    return s, np.ascontiguousarray(P)


def beyond_series(k):
    s = scenario(k)
    P = s["P"].copy()
    P[2, 4, 4] += 17.0                                           # 4.1 rad
    return s, np.ascontiguousarray(P)


ONE, TWO, MANY = 0, 2, 5                                         # the filters of the pass-count case


def pass_counts(k):
    s = scenario(k)
    P = s["P"].copy()
    P[ONE] *= 1e-6
    P[MANY, all_rot_rows(k), all_rot_rows(k)] += 1.0             # 1 rad in every block,
    s["z"] = s["z"].copy()
    s["z"][MANY] += 0.3                                          # and a larger innovation: the reference starts further off
    return s, np.ascontiguousarray(P)


def twin_passes(s, P, b):
    """Passes of the manifold mean in the first step's update, by the numpy twin of the oracle."""
    k, u = s["k"], s["u"][b]
    flt = npc.Msckf(k, s["mean"][b], P[b])
    seen, plain = [], flt.man.mean

    def recording(X):
        ref, it = plain(X)
        seen.append(it)
        return ref, it

    flt.man.mean = recording                                     # (predict takes its mean on a manifold of its own)
    flt.predict(lambda x: npc.pm_delta_pose(x, u[0:3], u[3:7], u[7:10], u[10:13]), s["Q"])
    flt.update(s["z"][b], lambda x: npc.mm_feature_proj(x, s["feat"][b]), s["R"])
    assert len(seen) == 1
    return seen[0]


def run_and_compare(slk, s, P, label):
    k, N, lay = s["k"], s["N"], o.layout(o.MULTI, s["k"])
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
    assert (st & ~slk.ST_ALL_REJECTED == 0).all()
    np.testing.assert_array_equal(tot, oc)
    for b in range(B):
        assert errs[b][0] <= TOL and errs[b][1] <= TOL, (b, errs[b])


@pytest.mark.parametrize("k", SHAPES)
def test_small_rotations_every_wave_on_the_direct_series(slk, k):
    s, P = small_rotations(k)
    L = np.linalg.cholesky(P)
    assert np.abs(L[:, all_rot_rows(k), :]).max() < 0.1          # the case is what it says: far below 1 rad
    run_and_compare(slk, s, P, "small")


@pytest.mark.parametrize("k", SHAPES)
def test_mixed_waves_take_different_branches(slk, k):
    s, P = mixed_waves(k)
    L = np.linalg.cholesky(P)
    for b, blk in ((1, 0), (4, k)):
        col = np.linalg.norm(L[b][rot_rows(k, blk), :], axis=0).max()
        assert 1.0 < col < 4.0, (b, col)
    for b in (0, 2, 3, 5):
        assert np.linalg.norm(L[b][all_rot_rows(k), :], axis=0).max() < 0.5, b
    run_and_compare(slk, s, P, "mixed")


@pytest.mark.parametrize("k", SHAPES)
def test_beyond_the_series_goes_to_the_general_body(slk, k):
    s, P = beyond_series(k)
    L = np.linalg.cholesky(P[2])
    assert np.linalg.norm(L[rot_rows(k, 0), :], axis=0).max() > 4.0
    run_and_compare(slk, s, P, "beyond")


@pytest.mark.parametrize("k", SHAPES)
def test_different_pass_counts_in_one_launch(slk, k):
    s, P = pass_counts(k)
    got = {b: twin_passes(s, P, b) for b in (ONE, TWO, MANY)}
    print(f"k={k} passes of the twin: {got}")
    assert got[ONE] == 1 and got[TWO] == 2 and got[MANY] > 2, got
    run_and_compare(slk, s, P, "passes")
