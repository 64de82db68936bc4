"""Route-by-route GPU parity: every branch launch_msckf / launch_usckf (csrc/slk_api.hip) can take for a legal call, against
the fp64 CPU oracle.  Each test names the route and the launcher lines it targets.  The earlier suites exercise the
headline shapes; this module covers the batch sizes, state sizes, measurement models, noise layouts, rebuild precisions and
window operations that select the other instantiations:

  * Usckf unit shape at the bench's batch (lower-triangle steady state, factorisation inside the update kernel);
  * Usckf N = 36 .. 96 over every kernel boundary, each registered measurement model, the whole-vector gate, the
    functor path, and the shapes the LDS carve refuses;
  * Msckf N = 12 / 18 on both sides of the B <= 4096 predict-inside switch, and the closed form reading global P;
  * per-filter and dense, correlated Q and R on every R-reading route;
  * reduced-precision covariance rebuild on the small-state kernels;
  * a sliding window whose length crosses instantiations mid-trajectory.
Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
from oracle import np_check as npc
import scenarios as sc

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def mean_err(lay, a, b):
    return float(np.abs(o.boxminus(lay, a, b)).max())


def colmajor_P(Pflat, N):
    """The oracle's batch functions keep each filter's P column-major: [B, N*N] -> [B, N, N] row / column indexable."""
    return np.ascontiguousarray(np.transpose(Pflat.reshape(-1, N, N), (0, 2, 1)))


def ref_usckf(s, b, nfk, nfkl, P=None, mean=None):
    return o.Usckf(nfk=nfk, nfkl=nfkl, mean=s["mean"][b] if mean is None else mean,
                   P=s["P"][b] if P is None else P)


def pm_cv(u):
    return o.pm_const_velocity(u[0:3], u[3:6], u[6])


def pm_dp(u):
    return o.pm_delta_pose(u[0:3], u[3:7], u[7:10], u[10:13])


def check_batch_properties(P, M, quat_offsets, exact_symmetry=True):
    """Size-independent properties of a whole batch: finite, exactly symmetric read-out, SPD, unit quaternions."""
    assert np.isfinite(P).all() and np.isfinite(M).all()
    if exact_symmetry:
        np.testing.assert_array_equal(P, np.transpose(P, (0, 2, 1)))
    assert np.linalg.eigvalsh(0.5 * (P + np.transpose(P, (0, 2, 1)))).min() > 0
    q = np.stack([M[:, o_:o_ + 4] for o_ in quat_offsets], axis=1)
    np.testing.assert_allclose(np.linalg.norm(q, axis=-1), 1.0, atol=1e-12)


def sample_idx(B, seed):
    rng = np.random.default_rng(seed)
    mid = rng.choice(np.arange(16, B - 16), size=32, replace=False)
    return np.unique(np.r_[0:16, mid, B - 16:B])


# ------------------------------------------------------------------ table rows 1 and 8: Usckf unit shape, full batch
@pytest.mark.parametrize("B", [4096, 4097])
def test_usckf_unit_shape_full_batch(slk, B):
    """Row 1: N = 48, m = 3 at the bench's batch -- launch_usckf_split (slk_api.hip:427-487) with lower_only and the
    factorisation inside the update kernel (slk_usckf_fast.hpp); B = 4097 leaves a partial last wave of workgroups.
    Then cloning(STATEK_I) and setMeasurement(STATEK_L) on the lower-triangle state, and one more step."""
    nfk, nfkl, steps = 3, 9, 3
    s = sc.synthetic_usckf(B, seed=0x5EED1000 + B)
    N = s["N"]
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    for _ in range(steps):
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    check_batch_properties(P, M, (3, 16, 29))
    idx = sample_idx(B, B)
    om = np.ascontiguousarray(s["mean"][idx])
    oP = np.ascontiguousarray(np.transpose(s["P"][idx], (0, 2, 1))).reshape(len(idx), -1)
    assert o.usckf_step_batch(nfk, nfkl, steps, om, oP, np.ascontiguousarray(s["u"][idx]),
                              np.ascontiguousarray(s["z"][idx]), s["Q"], s["R"]) == 0
    oP = colmajor_P(oP, N)
    for j, b in enumerate(idx):
        assert rel(P[b], oP[j]) <= TOL, b
        assert mean_err(lay, M[b], om[j]) <= TOL, b
    # cloning + setMeasurement straight after lower-triangle steps (both copy blocks of both triangles), then a step
    z9, R9 = np.linspace(1.0, 2.6, 9), sc.dense_noise(9, scale=0.008, seed=3)
    f.cloning(slk.STATEK_I)
    f.setMeasurement(slk.STATEK_L, z9, R9)
    f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert f.N == 48 and (f.status() == 0).all()
    P2, M2 = f.PkAugmentedState(), f.muState()
    check_batch_properties(P2, M2, (3, 16, 29))
    for j, b in enumerate(idx[::4]):
        r = ref_usckf(s, b, nfk, nfkl, P=oP[4 * j], mean=om[4 * j])
        r.cloning(o.STATEK_I)
        r.set_measurement(o.STATEK_L, z9, R9)
        assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
        st, acc = r.update(s["z"][b], o.mm_vo_relative(), s["R"])
        assert st == 0 and acc == 1
        assert rel(P2[b], r.P) <= TOL, b
        assert mean_err(lay, M2[b], r.mean) <= TOL, b


def test_usckf_set_measurement_moves_n_across_kernels(slk):
    """Row 8: setMeasurement (slk_api.hip:1087-1116) moving N across the Usckf instantiations at B > 1, each followed by a
    fused step: 48 (split, unit shape) -> 54 (usckf_kernel<4>) -> 57 (m = 6) -> 90 (<6>) -> 69 (<5>) -> 66 (m = 3) -> 48
    (split, unit shape again, lower-triangle state)."""
    B = 6
    s = sc.synthetic_usckf(B, seed=0x5E7)
    rng = np.random.default_rng(8)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
    refs = [ref_usckf(s, b, 3, 9) for b in range(B)]
    # setMeasurement calls before each step; a growing feature-k block (STATEK) is followed by a STATEK_L call: the
    # reference reads the kept featuresk_l block at the offset of the NEW featuresk size (Usckf.hpp:335-342), which
    # leaves zero rows in the covariance when featuresk grows
    moves = [[], [(slk.STATEK_L, 15)], [(slk.STATEK, 6), (slk.STATEK_L, 15)], [(slk.STATEK_L, 48)], [(slk.STATEK_L, 27)],
             [(slk.STATEK, 3)], [(slk.STATEK_L, 9)]]
    for calls in moves:
        for mode, n in calls:
            zs = rng.uniform(1, 4, n)
            Rs = sc.dense_noise(n, scale=0.01, seed=n)
            f.setMeasurement(mode, zs, Rs)
            for r in refs:
                r.set_measurement(mode, zs, Rs)
        P, M = f.PkAugmentedState(), f.muState()
        for b, r in enumerate(refs):
            assert rel(P[b], r.P) <= TOL and mean_err(r.lay, M[b], r.mean) <= TOL, (f.N, b)
        nfk = refs[0].lay.nfk
        assert f.N == refs[0].N
        lay = refs[0].lay
        # a measurement consistent with the mean
        z = np.array([npc.mm_vo_relative(r.mean, nfk) for r in refs]) + rng.normal(0, 0.05, (B, nfk))
        R = sc.dense_noise(nfk, scale=0.01, seed=100 + nfk)
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], z, slk.MM_VO_RELATIVE, None, R)
        assert (f.status() == 0).all(), (f.N, f.status())
        P, M = f.PkAugmentedState(), f.muState()
        for b, r in enumerate(refs):
            assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
            st, acc = r.update(z[b], o.mm_vo_relative(), R)
            assert st == 0 and acc == 1
            assert rel(P[b], r.P) <= TOL, (f.N, b)
            assert mean_err(lay, M[b], r.mean) <= TOL, (f.N, b)
    assert f.N == 48


# ------------------------------------------------------------------ table rows 2 .. 7: Usckf shape sweep
# (nfk, nfkl) -> N = 36 + nfk + nfkl.  N <= 48: launch_usckf_split (three launches; N = 48 off the unit layout runs
# msckf_chol_kernel<3, 6> and the generic split update, slk_api.hip:464-480); N = 49..64: usckf_kernel<4>; 65..80: <5>;
# 81..96: <6> (slk_api.hip:501-503).
USCKF_SHAPES = [(0, 0), (3, 0), (6, 6), (3, 10), (3, 23), (3, 25), (6, 23), (9, 35), (12, 33), (9, 45), (12, 48)]
# Shapes whose LDS carve (carve_usckf, slk_usckf.hpp) exceeds the 160 KiB of a workgroup for m = nfk rows: the launcher
# refuses them (slk_api.hip:415, include/slk.h).  Value: the carve in KiB at m = nfk as carve_usckf computes it (the
# shapes that do launch get exactly their carve: 146.0 KiB at N = 96 with m = 3 / 4, 131.7 KiB at N = 90).
USCKF_LDS_REFUSED = {(12, 48): 162.0, (18, 36): 170.2, (24, 20): 165.4}


def _usckf_vo_chain(slk, s, nfk, nfkl, B):
    """predict alone, update alone, fused step (MM_VO_RELATIVE, no gate) against two oracle predict + update rounds."""
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"])
    Pp, Mp = f.PkAugmentedState(), f.muState()
    f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (f.status() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        for i in range(2):
            assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
            if i == 0:
                assert rel(Pp[b], r.P) <= TOL and mean_err(lay, Mp[b], r.mean) <= TOL, ("predict", b)
            st, acc = r.update(s["z"][b], o.mm_vo_relative(), s["R"])
            assert st == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, ("step", b)


def _usckf_vo_gated(slk, s, nfk, nfkl, B):
    """Whole-vector chi-square gate with nfk degrees of freedom (Usckf.hpp:262-302); filter 1 pushed out."""
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    rng = np.random.default_rng(nfk + nfkl)
    z = np.array([npc.mm_vo_relative(x, nfk) for x in s["mean"]]) + rng.normal(0, 0.02, (B, nfk))
    z[1] += 5.0
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.update(z, slk.MM_VO_RELATIVE, None, s["R"], gate=nfk)
    st, out = f.status(), f.outliers()
    P, M = f.PkAugmentedState(), f.muState()
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        stc, acc = r.update(z[b], o.mm_vo_relative(), s["R"], gate_dof=nfk)
        # (the chi-square table of the reference ends at 9 degrees of freedom: a wider gate rejects every measurement)
        assert stc == 0 and acc == (0 if b == 1 or nfk > 9 else 1), b
        assert out[b] == 1 - acc and st[b] == (0 if acc else slk.ST_ALL_REJECTED), b
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


def _usckf_pose_position(slk, s, nfk, nfkl, B):
    """MM_POSE_POSITION of statek / statek_l / statek_i (slk_api.hip:563), fused with a predict."""
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    R = 0.01 * np.eye(3)
    for pose in (0, 1, 2):
        z = s["mean"][:, 13 * pose:13 * pose + 3] + np.array([0.05, -0.03, 0.02])
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], z, slk.MM_POSE_POSITION, np.array([float(pose)]), R)
        assert (f.status() == 0).all(), pose
        P, M = f.PkAugmentedState(), f.muState()
        for b in range(B):
            r = ref_usckf(s, b, nfk, nfkl)
            assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
            st, acc = r.update(z[b], o.mm_pose_position(pose), R)
            assert st == 0 and acc == 1
            assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, (pose, b)


def _usckf_feature_proj(slk, s, nfk, nfkl, B):
    """MM_FEATURE_PROJ with 2 features (statek and statek_i), update alone."""
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    feat, z = sc.usckf_features(s["mean"], seed=nfk + nfkl)
    R = 0.01 * np.eye(4)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.update(z, slk.MM_FEATURE_PROJ, feat, R)
    assert (f.status() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        st, acc = r.update(z[b], o.mm_feature_proj(feat[b]), R)
        assert st == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


def _usckf_functor_path(slk, s, nfk, nfkl, B):
    """Tier B (predict_from_sigma / update_functor, the fused usckf_kernel<NT, 256> with `emit`) == registered models."""
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    a = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    b = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    a.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"])
    a.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    X = b.predict_sigma_points()
    Y = np.ascontiguousarray([[npc.pm_const_velocity(x, s["u"][i, 0:3], s["u"][i, 3:6], s["u"][i, 6]) for x in X[i]]
                              for i in range(B)])
    Qc = np.ascontiguousarray(s["Q"].T)
    assert slk.load_library().slk_predict_from_sigma(b._h, Y.ctypes.data, Qc.ctypes.data, 0, slk.HOST) == 0
    b.update_functor(s["z"], lambda x: npc.mm_vo_relative(x, nfk), s["R"])
    assert (a.status() == 0).all() and (b.status() == 0).all()
    Pa, Pb, Ma, Mb = a.PkAugmentedState(), b.PkAugmentedState(), a.muState(), b.muState()
    for i in range(B):
        assert rel(Pb[i], Pa[i]) <= 1e-12 and mean_err(lay, Mb[i], Ma[i]) <= 1e-12, i


def _usckf_refused(slk, s, nfk, nfkl):
    """The LDS carve at m = nfk rows exceeds 160 KiB: update and step raise SlkError before any launch, the state is
    bit-identical afterwards and no status bit is set."""
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    with pytest.raises(slk.SlkError):
        f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    with pytest.raises(slk.SlkError):
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    with pytest.raises(slk.SlkError):
        f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"], gate=nfk)
    np.testing.assert_array_equal(f.PkAugmentedState(), s["P"])
    np.testing.assert_array_equal(f.muState(), s["mean"])
    assert (f.status() == 0).all()


@pytest.mark.parametrize("nfk,nfkl", USCKF_SHAPES, ids=[f"N{36 + a + b}-nfk{a}-nfkl{b}" for a, b in USCKF_SHAPES])
def test_usckf_shape_sweep(slk, nfk, nfkl):
    """Rows 2 .. 7: Usckf N = 36 .. 96 over every kernel boundary, m = nfk in {3, 6, 9, 12}: predict alone, update alone,
    fused step; MM_VO_RELATIVE with the gate off and on (slk_api.hip:561); MM_POSE_POSITION of each pose (:563);
    MM_FEATURE_PROJ; at N = 62 and 90 the functor path; the shapes the LDS carve refuses."""
    B = 4
    N = 36 + nfk + nfkl
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED2000 + N)
    if nfk:
        if (nfk, nfkl) in USCKF_LDS_REFUSED:
            _usckf_refused(slk, s, nfk, nfkl)
        else:
            _usckf_vo_chain(slk, s, nfk, nfkl, B)
            _usckf_vo_gated(slk, s, nfk, nfkl, B)
    _usckf_pose_position(slk, s, nfk, nfkl, B)
    _usckf_feature_proj(slk, s, nfk, nfkl, B)
    if N in (62, 90):
        _usckf_functor_path(slk, s, nfk, nfkl, B)


@pytest.mark.parametrize("nfk,nfkl", [(18, 36), (24, 20)])
def test_usckf_lds_limit_refuses_wide_measurements(slk, nfk, nfkl):
    """Legal shapes at or below N = 96 whose m = nfk measurement block takes the carve past 160 KiB (slk_api.hip:415):
    refused with SlkError and the state untouched; the handle keeps working for a narrower model (pose position)."""
    B = 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED3000 + nfk)
    _usckf_refused(slk, s, nfk, nfkl)
    _usckf_pose_position(slk, s, nfk, nfkl, B)


# ------------------------------------------------------------------ table rows 9 and 10: Msckf N = 12 / 18, large batches
@pytest.mark.parametrize("k,B", [(0, 4096), (0, 4097), (0, 8192), (1, 4096), (1, 4097), (1, 8192)])
def test_msckf_small_state_large_batch(slk, k, B):
    """Rows 9 / 10: `inside` at slk_api.hip:373 -- B <= 4096 runs predict inside the one-wave step kernel (the closed form
    of k = 0 reads the predicted block pred12 from LDS), B > 4096 launches msckf_predict_kernel on its own and the step
    kernel reads the predicted state from memory (closed form from global P, slk_kernels.hpp:2187-2207).  k = 0: 3-row
    position fix of pose 0, ungated; k = 1: one 2-D feature, gate on."""
    s = sc.synthetic_msckf(B, k, m=2, seed=0x5EED4000 + B + k)
    lay = o.layout(o.MULTI, k)
    steps = 2
    if k == 0:
        z, mm, par, R, gate = s["mean"][:, 0:3] + 0.05, slk.MM_POSE_POSITION, np.array([0.0]), 0.01 * np.eye(3), 0
    else:
        z, mm, par, R, gate = s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"], 1
    f = slk.Msckf(s["mean"], s["P"])
    tot = np.zeros(B, dtype=np.int64)
    for _ in range(steps):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], z, mm, par, R, gate=gate)
        tot += f.outliers()
    st = f.status()
    assert (st & ~slk.ST_ALL_REJECTED == 0).all()
    P, M = f.getPk(), f.muState()
    # (as test_cfg2_*: the read-out of N = 18 is symmetric to rounding, not bit for bit)
    check_batch_properties(P, M, (3,) + tuple(13 + 7 * c + 3 for c in range(k)), exact_symmetry=(k == 0))
    for b in sample_idx(B, B + k):
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        no_tot = 0
        for _ in range(steps):
            assert r.predict(pm_dp(s["u"][b]), s["Q"]) == 0
            model = o.mm_pose_position(0) if k == 0 else o.mm_feature_proj(s["feat"][b])
            stc, no = r.update(z[b], model, R, gate=bool(gate))
            assert stc == 0
            no_tot += no
        assert tot[b] == no_tot, b
        assert rel(P[b], r.P) <= TOL, b
        assert mean_err(lay, M[b], r.mean) <= TOL, b


def test_msckf_position_fix_reads_global_P(slk):
    """Row 10: the N = 12 closed form (msckf_step_kernel<1, 64, 0, 3>) with the moments read from global P -- an update
    alone, and a predict followed by a separate update -- against the oracle, with per-filter dense R (r_stride = 9)."""
    B, k = 64, 0
    s = sc.synthetic_msckf(B, k, m=2, seed=0x5EED5000)
    lay = o.layout(o.MULTI, k)
    z = s["mean"][:, 0:3] + np.array([0.05, -0.02, 0.03])
    R = sc.dense_noise(3, B=B, scale=0.01, seed=5)
    f = slk.Msckf(s["mean"], s["P"])
    f.update(z, slk.MM_POSE_POSITION, np.array([0.0]), R, gate=0)
    g = slk.Msckf(s["mean"], s["P"])
    g.predict(slk.PM_DELTA_POSE, s["u"], s["Q"])
    g.update(z, slk.MM_POSE_POSITION, np.array([0.0]), R, gate=0)
    assert (f.status() == 0).all() and (g.status() == 0).all()
    Pf, Mf, Pg, Mg = f.getPk(), f.muState(), g.getPk(), g.muState()
    for b in range(B):
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        assert r.update(z[b], o.mm_pose_position(0), R[b], gate=False) == (0, 0)
        assert rel(Pf[b], r.P) <= TOL and mean_err(lay, Mf[b], r.mean) <= TOL, ("update", b)
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        assert r.predict(pm_dp(s["u"][b]), s["Q"]) == 0
        assert r.update(z[b], o.mm_pose_position(0), R[b], gate=False) == (0, 0)
        assert rel(Pg[b], r.P) <= TOL and mean_err(lay, Mg[b], r.mean) <= TOL, ("predict, update", b)


# ------------------------------------------------------------------ table rows 11 and 12: per-filter, dense noise
# (route id, filter kind, k (Msckf), measurement rows, batch); the R reads: slk_step_fast.hpp:625 (exact k = 4 .. 8, m = 8),
# slk_kernels.hpp:1488 (moments of the generic bodies), :2187 (N = 12 closed form), slk_usckf_fast.hpp:120 (unit-shape
# Usckf, lower triangle of R), slk_general.hpp:179 (N > 208)
NOISE_ROUTES = [("k8-m8-exact", "msckf", 8, 8, 6), ("k5-m8-exact", "msckf", 5, 8, 6), ("k8-m6-general", "msckf", 8, 6, 6),
                ("k0-m3-closed-form", "msckf", 0, 3, 6), ("usckf-unit-fast", "usckf", None, 3, 6),
                ("k12-m8-big", "msckf", 12, 8, 4), ("k33-m8-global", "msckf", 33, 8, 2), ("k8-m20-two-tile-S", "msckf", 8, 20, 4)]


@pytest.mark.parametrize("route,kind,k,m,B", NOISE_ROUTES, ids=[r[0] for r in NOISE_ROUTES])
def test_per_filter_dense_noise(slk, route, kind, k, m, B):
    """Rows 11 / 12: dense, correlated Q and R with a 10:1 spread of variances, three ways -- shared (stride 0), per filter
    and identical (q_stride = 144, r_stride = m*m: bit-identical to shared), per filter and different (against the
    oracle) -- and a shared 1-D u against the same row tiled B times (bit-identical).  Two fused steps."""
    steps = 2
    Qs, Rs = sc.dense_noise(12, scale=0.01, seed=11), sc.dense_noise(m, scale=0.01, seed=12)
    Qp, Rp = sc.dense_noise(12, B=B, scale=0.01, seed=13), sc.dense_noise(m, B=B, scale=0.01, seed=14)
    if kind == "usckf":
        s = sc.synthetic_usckf(B, seed=0x5EED6000)
        lay = o.layout(o.AUGMENTED, 0, 3, 9)
        z, mm, par, gate = s["z"], slk.MM_VO_RELATIVE, None, 0
        new = lambda: slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)          # noqa: E731
        read = lambda f: (f.PkAugmentedState(), f.muState())                     # noqa: E731
        pm, pmodel = slk.PM_CONST_VELOCITY, pm_cv
    else:
        s = sc.synthetic_msckf(B, k, m=(m if k else 2), seed=0x5EED6000 + k + m)
        lay = o.layout(o.MULTI, k)
        if k == 0:
            z, mm, par, gate = s["mean"][:, 0:3] + 0.04, slk.MM_POSE_POSITION, np.array([0.0]), 0
        else:
            z, mm, par, gate = s["z"], slk.MM_FEATURE_PROJ, s["feat"], 1
        new = lambda: slk.Msckf(s["mean"], s["P"])                               # noqa: E731
        read = lambda f: (f.getPk(), f.muState())                                # noqa: E731
        pm, pmodel = slk.PM_DELTA_POSE, pm_dp

    def run(u, Q, R):
        f = new()
        tot = np.zeros(B, dtype=np.int64)
        for _ in range(steps):
            f.step(pm, u, Q, z, mm, par, R, gate=gate)
            tot += f.outliers()
        return (*read(f), f.status(), tot)

    def oracle(b, Q, R):
        if kind == "usckf":
            r = ref_usckf(s, b, 3, 9)
            model = o.mm_vo_relative()
        else:
            r = o.Msckf(k, s["mean"][b], s["P"][b])
            model = o.mm_pose_position(0) if k == 0 else o.mm_feature_proj(s["feat"][b])
        stc, no_tot = 0, 0
        for _ in range(steps):
            assert r.predict(pmodel(s["u"][b]), Q) == 0
            if kind == "usckf":
                st, acc = r.update(z[b], model, R)
                no = 1 - acc
            else:
                st, no = r.update(z[b], model, R, gate=bool(gate))
            stc |= st
            no_tot += no
        return r, stc, no_tot

    shared = run(s["u"], Qs, Rs)
    tiled = run(s["u"], np.ascontiguousarray(np.broadcast_to(Qs, (B, 12, 12))),
                np.ascontiguousarray(np.broadcast_to(Rs, (B, m, m))))
    for x, y in zip(shared, tiled):
        np.testing.assert_array_equal(x, y)
    perf = run(s["u"], Qp, Rp)
    for (P, M, st, tot), per_filter in ((shared, False), (perf, True)):
        for b in range(B):
            r, stc, no = oracle(b, Qp[b] if per_filter else Qs, Rp[b] if per_filter else Rs)
            assert stc == 0 and st[b] & ~slk.ST_ALL_REJECTED == 0, (per_filter, b)
            assert tot[b] == no, (per_filter, b)
            assert rel(P[b], r.P) <= TOL, (per_filter, b)
            assert mean_err(lay, M[b], r.mean) <= TOL, (per_filter, b)
    # a shared 1-D process input == the same row tiled over the batch
    one = run(s["u"][0], Qs, Rs)
    rows = run(np.ascontiguousarray(np.tile(s["u"][0], (B, 1))), Qs, Rs)
    for x, y in zip(one, rows):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ table row 13: reduced-precision rebuild, small states
@pytest.mark.parametrize("k", [0, 1, 4, 8])
def test_reduced_precision_rebuild_on_small_states(slk, k):
    """Row 13: set_rebuild_precision(1 | 2) on the non-big kernels (NT <= 4; slk_kernels.hpp:3120, :3235), as
    test_cfg5_rebuild_precisions_against_oracle does for N = 198 / 204: fp32 within 1e-6 and bf16 within 2e-2 of max |P|,
    really reduced (> 1e-11), the mean within TOL, the outlier counts unchanged."""
    B = 4
    m = {0: 3, 1: 2, 4: 8, 8: 8}[k]
    s = sc.synthetic_msckf(B, k, m=(m if k else 2), seed=0x5EED7000 + k)
    lay = o.layout(o.MULTI, k)
    if k == 0:
        z, mm, par, R, gate = s["mean"][:, 0:3] + 0.05, slk.MM_POSE_POSITION, np.array([0.0]), 0.01 * np.eye(3), 0
    else:
        z, mm, par, R, gate = s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"], 1
    refs = []
    for b in range(B):
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        assert r.predict(pm_dp(s["u"][b]), s["Q"]) == 0
        st, no = r.update(z[b], o.mm_pose_position(0) if k == 0 else o.mm_feature_proj(s["feat"][b]), R, gate=bool(gate))
        assert st == 0
        refs.append((r, no))
    for mode, bound in ((0, TOL), (1, 1e-6), (2, 2e-2)):
        f = slk.Msckf(s["mean"], s["P"])
        f.set_rebuild_precision(mode)
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], z, mm, par, R, gate=gate)
        assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
        np.testing.assert_array_equal(f.outliers(), [no for _, no in refs])
        Pg, Mg = f.getPk(), f.muState()
        worst = max(rel(Pg[b], refs[b][0].P) for b in range(B))
        assert worst <= bound, (mode, worst)
        if mode:
            assert worst > 1e-11, (mode, worst)
        for b in range(B):
            assert mean_err(lay, Mg[b], refs[b][0].mean) <= TOL, (mode, b)


# ------------------------------------------------------------------ table row 14: window across instantiations
def test_msckf_window_trajectory_across_instantiations(slk):
    """Row 14: 12 steps of clone_pose(), a fused step with fresh features, then drop_clone(0) as needed: the step runs at
    k = 6, 7, 8, 9, 10, 10, 10, 9, 8, 7, 6, 6 -- NT 3 -> 4 -> 5 and back, exact m = 8 shapes (k = 6 .. 8) <-> big kernels
    (k = 9, 10), lower-triangle state and the per-k rotation tables (slk_api.hip:249-255, :1118-1136) in between.  The
    oracle applies the same index manipulation in numpy and steps with msckf_step_batch.  A freshly pushed clone is
    singular until the predict of the following fused step adds Q to the pose block."""
    B, m = 16, 8
    k_steps = [6, 7, 8, 9, 10, 10, 10, 9, 8, 7, 6, 6]
    k = k_steps[0] - 1
    s = sc.synthetic_msckf(B, k, m=m, seed=0x5EED8000)
    rng = np.random.default_rng(14)
    f = slk.Msckf(s["mean"], s["P"])
    mean, P = s["mean"].copy(), s["P"].copy()
    for t, ks in enumerate(k_steps):
        # push: the new clone is the current pose, its rows / columns copy the pose's
        N, Nq = 12 + 6 * k, 13 + 7 * k
        f.clone_pose()
        src = np.concatenate([np.arange(N), np.arange(6)])
        P = P[:, src][:, :, src]
        mean = np.concatenate([mean, mean[:, 0:7]], axis=1)
        k += 1
        assert k == ks and f.N == 12 + 6 * k
        feat, z = sc.msckf_features(mean, k, m // 2, rng)
        u = s["u"].copy()
        u[:, 0:3] += rng.normal(0, 0.02, (B, 3))
        f.step(slk.PM_DELTA_POSE, u, s["Q"], z, slk.MM_FEATURE_PROJ, feat, s["R"])
        N = 12 + 6 * k
        Pf = np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(B, -1)
        st, out = o.msckf_step_batch(k, m, 1, mean, Pf, u, feat, z, s["Q"], s["R"])
        assert st == 0, t
        P = colmajor_P(Pf, N)
        assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all(), t
        np.testing.assert_array_equal(f.outliers(), out)
        lay = o.layout(o.MULTI, k)
        Pg, Mg = f.getPk(), f.muState()
        gm = Mg
        for b in range(B):
            assert rel(Pg[b], P[b]) <= TOL, (t, k, b)
            assert mean_err(lay, Mg[b], mean[b]) <= TOL, (t, k, b)
        # drop the oldest clones until the next step's window length (after its push) is reached
        k_next = k_steps[t + 1] if t + 1 < len(k_steps) else k
        while k > k_next - 1 and t + 1 < len(k_steps):
            N, Nq = 12 + 6 * k, 13 + 7 * k
            f.drop_clone(0)
            keep_t = np.concatenate([np.arange(12), np.arange(18, N)])
            keep_s = np.concatenate([np.arange(13), np.arange(20, Nq)])
            P, mean, gm = P[:, keep_t][:, :, keep_t], np.ascontiguousarray(mean[:, keep_s]), gm[:, keep_s]
            k -= 1
            np.testing.assert_array_equal(f.muState(), gm)
    assert k == 6
