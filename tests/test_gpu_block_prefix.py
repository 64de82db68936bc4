"""The exact-shape Msckf update (k = 4 .. 8, m = 8; csrc/slk_step_fast.hpp) takes the prefix sums G_j = sum_{k < j} a_k a_k^T
of the factor update (a_k = 1/2 dZ_k, 8 x 8 symmetric, one per column j) in BLOCKS of four columns: the base of every block
is the running accumulator of an MFMA chain over the k-steps of dZ (fast_prefix_blocks, parked in the dead Yp rows), each
lane adds the outer products of the up-to-three columns before it inside its block (fast_prefix_tail: a neighbour outside the
block is replaced by the all-zero column 63 of dZ), and the factor 1/4 goes into T_j = S - 1/4 (4 G_j).  The general body keeps
its 36 wave scans (ldm_prefix).  What the block form could lose is checked here against the oracle's batch step:

  * every shape: k = 4 .. 8 -- N mod 4 = 0 and 2, three and four tiles, 9 .. 15 blocks, and at N = 42 / 54 (k = 5, 7) a last
    block that is half live (columns N, N + 1 of dZ are zero; dead lanes beyond it take the base of that block);
  * where dZ is nonzero: k = 8 and k = 5 with all four features on pose 0 (columns 0 .. 5 only: every later base equals
    the total, tails are zero), all on the newest clone (the last live lanes N - 3 .. N - 1 take a full tail) and on poses
    [0, 3, 5, k];
  * the gate: k = 8 with one and with two measurement blocks rejected -- the prefix is formed before the gate, of all eight
    rows, and the masked set-up of T_j consumes it;
  * the block form against the scan form with no oracle in between: the fast path and the general body of the same
    instantiation (slk_update_selected with every row kept) on the device, k = 5 and 8;
  * a strong downdate: k = 8 with R (and the measurement noise) scaled by 1e-4, where T_j = S - G_j cancels most of S and
    the smallest d_j of chol(I - B B^T) falls to 1.3e-4 (first update, from P- and P+ of the numpy twin; 0.42 at scale 1).
    The scale was chosen on the CPU: the C oracle (oracle/slk_oracle.c) and its numpy twin (oracle/np_check.py) agree on
    these inputs after the three steps to P 8.3e-15 / mean 1.8e-15 at scale 1, 1.6e-14 / 1.8e-15 at 1e-2 (min d_j 7.5e-3),
    1.6e-14 / 1.8e-15 at 1e-3 (8.8e-4) and 3.0e-14 / 4.3e-15 at 1e-4 (required: TOL / 10 = 1e-10), no outliers in
    either; 1e-4 is the smallest scale that was tried;
  * a mean z-bar far from Z_0: k = 8 with the rotation variance of every block inflated to columns of one radian (as
    tests/test_gpu_parity.py and tests/test_gpu_matrix_trim.py do) -- the gate decides on the innovation z - z-bar, and the
    outliers must be the oracle's.
Every case: status == 0, outliers equal to the oracle's, P exactly symmetric.  B = 8 filters, 3 steps; TOL = 1e-9 and the
helpers of tests/test_gpu_routes.py.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
import test_gpu_caller_gate as cg
from test_gpu_routes import TOL, colmajor_P, mean_err, rel

pytestmark = pytest.mark.gpu
B, STEPS, M = 8, 3, 8
DOWNDATE_SCALE = 1e-4


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def scenario(k, poses=None, meas_sigma=0.05):
    """The synthetic scenario, with the four features observed from the given poses (0 = the current state, c = clone c)."""
    s = sc.synthetic_msckf(B, k, m=M, seed=0xB10C0000 + k, meas_sigma=meas_sigma)
    if poses is None:
        return s
    rng = np.random.default_rng(0xB10C1000 + 16 * k + sum(poses))
    mean, feat, z = s["mean"], s["feat"].copy(), s["z"].copy()
    for j, c in enumerate(poses):
        at = 0 if c == 0 else 13 + 7 * (c - 1)
        local = np.concatenate([rng.uniform(-1, 1, (B, 2)), rng.uniform(4, 8, (B, 1))], axis=1)
        feat[:, j, 0:3] = mean[:, at:at + 3] + sc.quat_rotate(mean[:, at + 3:at + 7], local)
        feat[:, j, 3] = c
        z[:, 2 * j:2 * j + 2] = local[:, 0:2] / local[:, 2:3] + rng.normal(0, meas_sigma, (B, 2))
    s["feat"], s["z"] = np.ascontiguousarray(feat), np.ascontiguousarray(z)
    return s


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
    assert (st == 0).all()
    np.testing.assert_array_equal(tot, oc)
    for b in range(B):
        assert errs[b][0] <= TOL and errs[b][1] <= TOL, (b, errs[b])
        np.testing.assert_array_equal(Pg[b], Pg[b].T)
    return oc


@pytest.mark.parametrize("k", [4, 5, 6, 7, 8])
def test_default_scenario_every_shape(slk, k):
    s = scenario(k)
    run_and_compare(slk, s, s["P"], "default")


@pytest.mark.parametrize("k,poses", [(8, [0, 0, 0, 0]), (8, [8, 8, 8, 8]), (8, [0, 3, 5, 8]),
                                     (5, [0, 0, 0, 0]), (5, [5, 5, 5, 5]), (5, [0, 3, 5, 5])])
def test_feature_poses_move_the_nonzero_columns(slk, k, poses):
    s = scenario(k, poses)
    run_and_compare(slk, s, s["P"], f"poses {poses}")


@pytest.mark.parametrize("nrej", [1, 2])
def test_prefix_is_consumed_by_the_masked_set_up(slk, nrej):
    s = scenario(8)
    z = s["z"].copy()
    z[:, 2:4] += 0.8                                             # feature 1 far outside the gate, in every step
    if nrej == 2:
        z[:, 6:8] -= 0.9                                         # and feature 3
    s["z"] = np.ascontiguousarray(z)
    oc = run_and_compare(slk, s, s["P"], f"{nrej} blocks rejected")
    assert (oc >= STEPS * nrej).all() and (oc < STEPS * 4).all(), oc


@pytest.mark.parametrize("k", [5, 8])
def test_block_form_against_the_scans_of_the_general_body(slk, k):
    s = scenario(k)
    lay = o.layout(o.MULTI, k)
    fast = slk.Msckf(s["mean"], s["P"])
    rsel = cg.make_rowsel([list(range(M))] * B, [0] * B, M)
    for it in range(STEPS):
        M0, P0 = fast.muState(), fast.getPk()
        gen = slk.Msckf(M0, P0)                                  # each step from the fast path's state: one update apart
        fast.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        gen.predict(slk.PM_DELTA_POSE, s["u"], s["Q"])
        assert cg.selected(slk, gen, slk.MM_FEATURE_PROJ, s["feat"], s["z"], s["R"], rsel) == 0
        assert (fast.status() == 0).all() and (gen.status() == 0).all()
        np.testing.assert_array_equal(fast.outliers(), 0)        # nothing gated out: both use the same eight rows
        Pf, Mf, Pg, Mg = fast.getPk(), fast.muState(), gen.getPk(), gen.muState()
        errs = [(rel(Pf[b], Pg[b]), mean_err(lay, Mf[b], Mg[b])) for b in range(B)]
        print(f"k={k} step {it}: fast path against the general body: P {max(e[0] for e in errs):.2e} mean {max(e[1] for e in errs):.2e}")
        for b in range(B):
            assert errs[b][0] <= TOL and errs[b][1] <= TOL, (it, b, errs[b])
            np.testing.assert_array_equal(Pf[b], Pf[b].T)
    # and the fast path's three steps against the oracle's, outliers included
    run_and_compare(slk, s, s["P"], "against the oracle")


def test_strong_downdate(slk):
    """R and the measurement noise scaled by DOWNDATE_SCALE = 1e-4 (see the module docstring for how it was chosen: the C
    oracle and its numpy twin agree to P 3.0e-14 / mean 4.3e-15 <= TOL / 10 on this input; min d_j = 1.3e-4)."""
    s = scenario(8, meas_sigma=0.05 * np.sqrt(DOWNDATE_SCALE))
    s["R"] = DOWNDATE_SCALE * s["R"]
    run_and_compare(slk, s, s["P"], f"R x {DOWNDATE_SCALE:g}")


def test_mean_of_z_far_from_the_centre_point(slk):
    k = 8
    s = scenario(k)
    P = s["P"].copy()
    rot = [t for b in range(k + 1) for t in range(9 + 6 * b if b else 3, (9 + 6 * b if b else 3) + 3)]
    P[:, rot, rot] += 1.0                                        # columns of 1 rad in every rotation block
    P = np.ascontiguousarray(P)
    run_and_compare(slk, s, P, "rotation columns of one radian")
