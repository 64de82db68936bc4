"""The exact-shape Msckf update (k = 4 .. 8, m = 8; csrc/slk_step_fast.hpp) forms every tile M(Kb, J) of the factor update
L' = L M once per wave -- output tiles are given to the waves by tile column (fast_ldm_wave) -- and adds the rank-2 term
p d0^T + d0 p^T of the covariance rebuild as one more k-step of the even-part tiles in the rotation-row space
(fast_ee_rank2) instead of one per N x N output tile.  What that could lose is checked here, against the oracle's batch step:

  * the map of both tile counts with nothing skipped: k = 4 (NT = 3, one even-part tile), k = 6 (NT = 3, two), k = 7 and
    k = 8 (NT = 4), features on the newest poses (JB = NT - 1, JB = the last tile column a measurement row depends on);
  * each wave's skip of tile columns and k-blocks beyond JB: k = 8 with the features on pose 0 (the current state: columns
    0 .. 5, JB = 0 -- pose 1 already reaches column 17), on poses 1 .. 3 (JB = 1) and 4 .. 6 (JB = 2), and the same of the
    NT = 3 map at k = 6 (JB = 0, 1);
  * identity rows of M: k = 8 with one and with two measurement blocks pushed out of the gate;
  * a rank-2 term that is not negligible: the centre deviation d0 is of third order in the rotation columns and the
    correction delta together, so the rotation variance of every block is inflated (columns of the factor of one radian, as
    tests/test_gpu_parity.py and tests/test_gpu_mean_loop_trim.py do) and the measurement moved by 1 (inside the gate of the
    inflated S), for one and for two even-part tiles.  The term's share of P+ in the first update is measured on the numpy
    twin of the oracle (oracle/np_check.py), P+ - O O^T - E^ E^^T from the twin's own sigma points, and asserted of IT to
    be above 1e4 TOL (it is 5e-5 .. 8e-5): a wrong sign or p and d0 swapped on one side misses by that much.
Every case: status == 0, outliers equal to the oracle's, P exactly symmetric.  B = 8 filters, 3 steps; TOL = 1e-9 and the
helpers of tests/test_gpu_routes.py, as tests/test_gpu_mean_loop_trim.py.  Run with `pytest -m gpu` on an MI355X.
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


def last_tile_column(poses):
    """JB of the kernel: the tile column of the last column any measurement row depends on (pose c: rows 6 + 6 c .. 11 + 6 c,
    the current state rows 0 .. 5)."""
    return max((6 + 6 * c if c else 0) + 5 for c in poses) >> 4


def scenario(k, poses=None):
    """The synthetic scenario with the four features observed from the given poses (0 = the current state, c = clone c)."""
    s = sc.synthetic_msckf(B, k, m=M, seed=0x7A1E0000 + k)
    if poses is None:
        return s
    rng = np.random.default_rng(0x7A1E1000 + 16 * k + sum(poses))
    mean, feat, z = s["mean"], s["feat"].copy(), s["z"].copy()
    for j, c in enumerate(poses):
        at = 0 if c == 0 else 13 + 7 * (c - 1)
        local = np.concatenate([rng.uniform(-1, 1, (B, 2)), rng.uniform(4, 8, (B, 1))], axis=1)
        feat[:, j, 0:3] = mean[:, at:at + 3] + sc.quat_rotate(mean[:, at + 3:at + 7], local)
        feat[:, j, 3] = c
        z[:, 2 * j:2 * j + 2] = local[:, 0:2] / local[:, 2:3] + rng.normal(0, 0.05, (B, 2))
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


@pytest.mark.parametrize("k", [4, 6, 7, 8])
def test_features_on_the_newest_poses_nothing_skipped(slk, k):
    poses = [k, k - 1, k - 2, k - 3]
    assert last_tile_column(poses) == (12 + 6 * k + 15) // 16 - 1
    s = scenario(k, poses)
    run_and_compare(slk, s, s["P"], f"poses {poses}")


@pytest.mark.parametrize("k,poses,jb", [(8, [0, 0, 0, 0], 0), (8, [1, 2, 3, 1], 1), (8, [4, 5, 6, 4], 2),
                                        (6, [0, 0, 0, 0], 0), (6, [1, 2, 3, 1], 1)])
def test_tile_columns_beyond_the_last_measured_pose_are_skipped(slk, k, poses, jb):
    assert last_tile_column(poses) == jb
    s = scenario(k, poses)
    run_and_compare(slk, s, s["P"], f"poses {poses} (JB = {jb})")


@pytest.mark.parametrize("nrej", [1, 2])
def test_rejected_blocks_leave_identity_rows_in_m(slk, nrej):
    s = scenario(8)
    z = s["z"].copy()
    z[:, 2:4] += 0.8                                             # feature 1 far outside the gate, in every step
    if nrej == 2:
        z[:, 6:8] -= 0.9                                         # and feature 3
    s["z"] = np.ascontiguousarray(z)
    oc = run_and_compare(slk, s, s["P"], f"{nrej} blocks rejected")
    assert (oc >= STEPS * nrej).all() and (oc < STEPS * 4).all(), oc


def rank2_share(s, P, b):
    """max |p d0^T + d0 p^T| / max |P+| of the first step's update, from the sigma points of the numpy twin:
    P+ = 1/2 sum_i d_i d_i^T = O O^T + E^ E^^T + [the rank-2 term], o_j / e_j the odd / even part of the pair of column j,
    E^ = E - d_0 1^T, d_0 the deviation of the centre point."""
    k, u = s["k"], s["u"][b]
    flt = npc.Msckf(k, s["mean"][b], P[b])
    seen, plain = [], flt.man.cov

    def recording(mean, X):
        seen.append(np.array([flt.man.minus(x, mean) for x in X]))
        return plain(mean, X)

    flt.man.cov = recording                                      # (predict takes its covariance on a manifold of its own)
    flt.predict(lambda x: npc.pm_delta_pose(x, u[0:3], u[3:7], u[7:10], u[10:13]), s["Q"])
    flt.update(s["z"][b], lambda x: npc.mm_feature_proj(x, s["feat"][b]), s["R"])
    assert len(seen) == 1
    D = seen[0]
    d0, Dp, Dm = D[0], D[1::2], D[2::2]
    O, Eh = 0.5 * (Dp - Dm), 0.5 * (Dp + Dm) - d0[None, :]
    Pp = 0.5 * D.T @ D
    r2 = Pp - O.T @ O - Eh.T @ Eh
    p = Eh.sum(axis=0) + 0.5 * (len(d0) + 0.5) * d0
    form = np.outer(p, d0) + np.outer(d0, p)
    assert np.abs(r2 - form).max() <= 1e-12 * np.abs(Pp).max()   # the identity the kernel builds on, on the twin's numbers
    return float(np.abs(form).max() / np.abs(Pp).max())


@pytest.mark.parametrize("k", [4, 6, 8])
def test_rank2_term_with_a_large_centre_deviation(slk, k):
    s = scenario(k)
    P = s["P"].copy()
    rot = [t for b in range(k + 1) for t in range(9 + 6 * b if b else 3, (9 + 6 * b if b else 3) + 3)]
    P[1::2, rot, rot] += 1.0                                     # columns of 1 rad in every rotation block
    s["z"] = s["z"].copy()
    s["z"][1::2] += 1.0                                          # and a correction delta that is no longer small beside them
    P = np.ascontiguousarray(P)
    share = [rank2_share(s, P, b) for b in (1, 3)]
    print(f"k={k}: share of the rank-2 term in P+ (first update, numpy twin): {share}")
    assert min(share) > 1e4 * TOL, share
    run_and_compare(slk, s, P, "large centre deviation")
