"""The filter kernels refine the hardware seeds of 1 / sqrt(d) and 1 / a by ONE higher-order step (rsqrt_pivot: third order,
csrc/slk_kernels.hpp; rcp_refined: second order, csrc/slk_math.hpp) where they took two Newton steps.  The results differ in
the last bit or two of every inverse root and reciprocal; what that must not change is checked here against the fp64 CPU
oracle, on every caller of the two helpers:

  * fused Msckf steps on the exact-shape fast path (k = 4 and k = 8, m = 8), three in a row;
  * the same shapes with the covariance congruence-scaled, P <- D P D, by a diagonal whose entries span ten decades, so that
    the pivots of one factorisation cover twenty decades (update() alone meets all of them; in a fused step the predict
    first replaces the current state's block: twelve decades at k = 4, twenty at k = 8);
  * a covariance whose smallest eigenvalue is 1e-10 of the largest, next to healthy filters: status (with its
    factorisation flag ST_LLT_FAIL) as the oracle's for every filter, the neighbours in parity;
  * predict alone at N = 12 (chol_rows<12>, the SO(3) logarithm of the mean loop);
  * one step of the Usckf unit shape (N = 48, m = 3).

The fast path is established as tests/test_gpu_factor_padding.py establishes it: the shape (k = 4 .. 8, m = 8, default
configuration) selects msckf_step_kernel<NT, 256, k, 8>, and a filter stays on its fast path while every rotation column of
the factor is below 1 rad and the status is clean -- the scalings below leave the rotation rows at or below their
synthetic size.  Tolerance: TOL = 1e-9 of tests/test_gpu_routes.py, which holds the same calls to it.
Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
from test_gpu_routes import TOL, colmajor_P, mean_err, pm_dp, rel

pytestmark = pytest.mark.gpu
M = 8
SHAPES = [4, 8]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def row_scales(k, for_step):
    """The diagonal D, one entry per tangent row, 1e-6 .. 1e+4.  Rows that reach the measurement model keep their synthetic
    size or shrink (a pose spread of kilometres or a rotation spread of many turns would leave the domain in which the
    reference's own gate and mean loop behave): positions 1e-6 .. 1, rotations 1e-5 .. 1.  The rows the model never reads grow:
    the positions of the clones no feature is seen from (the four features of synthetic_msckf are seen from clones 0 .. 3)
    and, for update() alone, velocity and angular velocity of the current state.  Before a predict those six rows may only
    shrink: the reference's predict writes Q over their block and keeps their covariances with the clones, so grown ones
    leave a predicted matrix that is not positive definite (its LLT fails in the oracle too)."""
    d = np.ones(12 + 6 * k)
    d[0:3] = [1e-6, 1e-3, 1.0]
    d[3:6] = [1e-4, 1.0, 1e-2]
    d[6:12] = [1.0, 1e-6, 1e-2, 1e-4, 1e-3, 1e-5] if for_step else [1e4, 1e-6, 1e2, 1e-2, 1e3, 1e-5]
    small_pos = [1e-6, 1e-2, 1.0, 1e-4, 1e-5, 1e-1, 1e-3, 1.0, 1e-6]
    small_rot = [1e-5, 1.0, 1e-3, 1e-1, 1e-4, 1e-2, 1.0, 1e-5, 1e-3]
    grown_pos = [1e4, 1e-6, 1e2, 1e-4, 1e3, 1e-5, 1e1, 1e-3, 1e4]
    for c in range(k):
        t = 12 + 6 * c
        d[t:t + 3] = (grown_pos if c >= 4 else small_pos)[c % 7:c % 7 + 3]
        d[t + 3:t + 6] = small_rot[c % 7:c % 7 + 3]
    return d


def scaled_scenario(k, seed, for_step):
    s = sc.synthetic_msckf(8, k, m=M, seed=seed)
    d = row_scales(k, for_step)
    s["P"] = np.ascontiguousarray(s["P"] * d[None, :, None] * d[None, None, :])
    s["P"] = 0.5 * (s["P"] + np.transpose(s["P"], (0, 2, 1)))
    return s, d


def run_steps(slk, s, k, steps):
    """`steps` fused steps on the GPU and in the oracle -> (P, mean, status, outliers) of both."""
    B, N = s["mean"].shape[0], s["N"]
    f = slk.Msckf(s["mean"], s["P"])
    tot = np.zeros(B, dtype=np.int64)
    for _ in range(steps):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        tot += f.outliers()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    st, oc = o.msckf_step_batch(k, M, steps, om, oP, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    return (f.getPk(), f.muState(), f.status(), tot), (colmajor_P(oP, N), om, st, oc)


@pytest.mark.parametrize("k", SHAPES)
def test_fast_path_steps(slk, k):
    s = sc.synthetic_msckf(8, k, m=M, seed=0x5EEDA100 + k)
    lay = o.layout(o.MULTI, k)
    (P, Mg, st, tot), (oP, om, ost, oc) = run_steps(slk, s, k, 3)
    assert ost == 0 and (st & ~slk.ST_ALL_REJECTED == 0).all()      # clean status on the exact shape: the fast path's route
    worst_P = max(rel(P[b], oP[b]) for b in range(8))
    worst_m = max(mean_err(lay, Mg[b], om[b]) for b in range(8))
    print(f"k={k}: P {worst_P:.2e} mean {worst_m:.2e} outliers {tot} / {oc}")
    np.testing.assert_array_equal(tot, oc)
    assert worst_P <= TOL and worst_m <= TOL


@pytest.mark.parametrize("k", SHAPES)
def test_pivots_across_many_magnitudes_steps(slk, k):
    s, d = scaled_scenario(k, 0x5EEDA200 + k, True)
    lay = o.layout(o.MULTI, k)
    (P, Mg, st, tot), (oP, om, ost, oc) = run_steps(slk, s, k, 3)
    assert ost == 0 and (oc == 0).all()              # the scaling keeps the oracle itself clean
    assert (st == 0).all()
    np.testing.assert_array_equal(tot, oc)
    worst_P = max(rel(P[b], oP[b]) for b in range(8))
    worst_m = max(mean_err(lay, Mg[b], om[b]) for b in range(8))
    # (not asserted: the same difference with the scaling taken out again, entry (i, j) against d_i d_j)
    unscaled = max(float(np.abs((P[b] - oP[b]) / np.outer(d, d)).max()) for b in range(8))
    print(f"k={k}: diagonal of P0 {np.einsum('bii->bi', s['P']).min():.1e} .. {np.einsum('bii->bi', s['P']).max():.1e}; "
          f"P {worst_P:.2e} mean {worst_m:.2e}; D^-1 (P - P_oracle) D^-1 {unscaled:.2e}")
    assert worst_P <= TOL and worst_m <= TOL


@pytest.mark.parametrize("k", SHAPES)
def test_pivots_across_many_magnitudes_update(slk, k):
    """update() factors the covariance as given: all N pivots of the scaled matrix, 1e-14 .. 1e+6."""
    s, d = scaled_scenario(k, 0x5EEDA300 + k, False)
    lay = o.layout(o.MULTI, k)
    piv = np.concatenate([np.diag(o.cholesky_lower(s["P"][b])[0]) ** 2 for b in range(8)])
    assert piv.max() / piv.min() > 1e18
    f = slk.Msckf(s["mean"], s["P"])
    f.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    assert (f.status() == 0).all()
    P, Mg, out = f.getPk(), f.muState(), f.outliers()
    worst_P = worst_m = 0.0
    for b in range(8):
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert sto == 0 and no == 0 and out[b] == 0, b
        worst_P, worst_m = max(worst_P, rel(P[b], r.P)), max(worst_m, mean_err(lay, Mg[b], r.mean))
    print(f"k={k}: pivots {piv.min():.1e} .. {piv.max():.1e}; P {worst_P:.2e} mean {worst_m:.2e}")
    assert worst_P <= TOL and worst_m <= TOL


BARELY = (2, 5)


def barely_positive_definite(P, ratio=1e-10):
    """P - a w w^T with w the eigenvector of P's smallest eigenvalue restricted to the clone rows (so that the predict, which
    rewrites the current state's block, leaves the direction alone) and a found by bisection: smallest eigenvalue =
    ratio * largest."""
    lam, V = np.linalg.eigh(P)
    w = V[:, 0].copy()
    w[:12] = 0.0
    w /= np.linalg.norm(w)
    a_sing = 1.0 / float(w @ np.linalg.solve(P, w))          # P - a_sing w w^T is singular
    lo, hi = 0.0, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        Q = P - a_sing * (1.0 - mid) * np.outer(w, w)
        ev = np.linalg.eigvalsh(0.5 * (Q + Q.T))
        if ev[0] > ratio * ev[-1]:
            hi = mid
        else:
            lo = mid
    Q = P - a_sing * (1.0 - hi) * np.outer(w, w)
    return 0.5 * (Q + Q.T)


@pytest.fixture(scope="module")
def barely(request):
    out = {}
    for k in SHAPES:
        s = sc.synthetic_msckf(8, k, m=M, seed=0x5EEDA400 + k)
        for b in BARELY:
            s["P"][b] = barely_positive_definite(s["P"][b])
            ev = np.linalg.eigvalsh(s["P"][b])
            assert 0.5e-10 < ev[0] / ev[-1] < 2e-10
        out[k] = s
    return out


@pytest.mark.parametrize("k", SHAPES)
@pytest.mark.parametrize("call", ["update", "step"])
def test_barely_positive_definite_covariance(slk, barely, k, call):
    """update() factors the matrix as given: eigenvalue ratio 1e-10, positive definite with a margin of 1e6 roundings -- the
    oracle's LLT passes and so must the kernel's.  step() factors the predicted matrix: the predict rewrites the current
    state's block and keeps its covariances with the clones, which moves the weak direction to about +-1e-3 of the
    largest eigenvalue (printed) -- clearly positive for one of the two filters, clearly negative for the other, whose LLT
    fails in the oracle and must fail here.  Either way the status is the oracle's, filter by filter."""
    s = barely[k]
    lay = o.layout(o.MULTI, k)
    f = slk.Msckf(s["mean"], s["P"])
    if call == "step":
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    else:
        f.update(s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    st, out, P, Mg = f.status(), f.outliers(), f.getPk(), f.muState()
    for b in range(8):
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        if call == "step":
            assert r.predict(pm_dp(s["u"][b]), s["Q"]) == 0
            if b in BARELY:
                ev = np.linalg.eigvalsh(r.P)
                print(f"k={k} filter {b}: predicted covariance, smallest / largest eigenvalue {ev[0] / ev[-1]:.2e}")
        sto, no = r.update(s["z"][b], o.mm_feature_proj(s["feat"][b]), s["R"])
        assert int(st[b]) & ~slk.ST_ALL_REJECTED == sto, (b, int(st[b]), sto)      # (the oracle has no all-rejected bit)
        assert bool(st[b] & slk.ST_LLT_FAIL) == bool(sto & slk.ST_LLT_FAIL), b
        assert out[b] == no, b
        eP, em = rel(P[b], r.P), mean_err(lay, Mg[b], r.mean)
        if b in BARELY:
            print(f"k={k} {call} filter {b} (barely positive definite): status {int(st[b])}, P {eP:.2e} mean {em:.2e}")
        else:
            assert sto == 0 and eP <= TOL and em <= TOL, (b, eP, em)


def test_predict_alone_n12(slk):
    B = 8
    s = sc.synthetic_msckf(B, 0, m=2, seed=0x5EEDA500)
    lay = o.layout(o.MULTI, 0)
    f = slk.Msckf(s["mean"], s["P"])
    f.predict(slk.PM_DELTA_POSE, s["u"], s["Q"])
    assert (f.status() == 0).all()
    P, Mg = f.getPk(), f.muState()
    for b in range(B):
        r = o.Msckf(0, s["mean"][b], s["P"][b])
        assert r.predict(pm_dp(s["u"][b]), s["Q"]) == 0
        assert rel(P[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, b


def test_usckf_unit_shape_step(slk):
    B, nfk, nfkl = 4, 3, 9
    s = sc.synthetic_usckf(B, seed=0x5EEDA600)
    N, lay = s["N"], o.layout(o.AUGMENTED, 0, nfk, nfkl)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    om, oP = s["mean"].copy(), np.ascontiguousarray(np.transpose(s["P"], (0, 2, 1))).reshape(B, -1)
    assert o.usckf_step_batch(nfk, nfkl, 1, om, oP, s["u"], s["z"], s["Q"], s["R"]) == 0
    oP = colmajor_P(oP, N)
    P, Mg = f.PkAugmentedState(), f.muState()
    for b in range(B):
        assert rel(P[b], oP[b]) <= TOL and mean_err(lay, Mg[b], om[b]) <= TOL, b
