"""Usckf with more than 96 state dimensions (N = 36 + nfk + nfkl > 96): the global-workspace predict kernel
(csrc/slk_usckf_general.hpp), every update-side call on the wide update kernel (csrc/slk_usckf_wide.hpp, launch_usckf_wide
in csrc/slk_api.hip) and setMeasurement past 96, against the fp64 CPU oracle with the helpers and the tolerance of
test_gpu_routes.py.  Every case here was refused with SlkError before N > 96 was supported.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
from oracle import np_check as npc
import scenarios as sc
import test_gpu_routes as routes

pytestmark = pytest.mark.gpu
TOL = routes.TOL
rel, mean_err, ref_usckf, pm_cv = routes.rel, routes.mean_err, routes.ref_usckf, routes.pm_cv

# (SLK_MM_VO_RELATIVE takes m = nfk rows in whole features of three: nfk = 30 is its widest update below MAXM = 32; the
# m = MAXM rows run through MM_FEATURE_PROJ with 16 features in test_usckf_large_maxm_rows)
LARGE_SHAPES = [(3, 58), (0, 64), (9, 60), (12, 60), (24, 72), (30, 98), (30, 130)]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def oracle_step_batch(s, idx, nfk, nfkl, steps):
    N = s["N"]
    om = np.ascontiguousarray(s["mean"][idx])
    oP = np.ascontiguousarray(np.transpose(s["P"][idx], (0, 2, 1))).reshape(len(idx), -1)
    st = o.usckf_step_batch(nfk, nfkl, steps, om, oP, np.ascontiguousarray(s["u"][idx]),
                            np.ascontiguousarray(s["z"][idx]), s["Q"], s["R"])
    return st, om, routes.colmajor_P(oP, N)


# ------------------------------------------------------------------ 1. shape sweep
@pytest.mark.parametrize("nfk,nfkl", LARGE_SHAPES, ids=[f"N{36 + a + b}-nfk{a}-nfkl{b}" for a, b in LARGE_SHAPES])
def test_usckf_large_shape_sweep(slk, nfk, nfkl):
    """N = 97 .. 196 (m up to MAXM): predict alone, update alone, fused step with MM_VO_RELATIVE (gate off, and on with
    nfk degrees of freedom: accepted at nfk <= 9, all rejected above, filter 1 pushed out); MM_POSE_POSITION of each
    pose; MM_FEATURE_PROJ."""
    B = 4
    N = 36 + nfk + nfkl
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED4000 + N)
    if nfk:
        routes._usckf_vo_chain(slk, s, nfk, nfkl, B)
        routes._usckf_vo_gated(slk, s, nfk, nfkl, B)
    routes._usckf_pose_position(slk, s, nfk, nfkl, B)
    routes._usckf_feature_proj(slk, s, nfk, nfkl, B)


@pytest.mark.parametrize("nfk,nfkl", [(30, 98), (30, 130)], ids=["N164", "N196"])
def test_usckf_large_maxm_rows(slk, nfk, nfkl):
    """m = MAXM = 32 rows: MM_FEATURE_PROJ with 16 features seen from all three poses, fused with a predict."""
    B = 4
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED4100 + nfkl)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    feat, z = sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(16)), seed=nfkl)
    R = 0.01 * np.eye(32)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], z, slk.MM_FEATURE_PROJ, feat, R)
    assert (f.status() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
        st, acc = r.update(z[b], o.mm_feature_proj(feat[b]), R)
        assert st == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


# ------------------------------------------------------------------ 2. full batch
def test_usckf_large_full_batch(slk):
    """N = 132, B = 1024, three fused steps: status 0, exactly symmetric SPD covariances, unit quaternions, 16 sampled
    filters against the oracle."""
    nfk, nfkl, B, steps = 24, 72, 1024, 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED5000)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    for _ in range(steps):
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    routes.check_batch_properties(P, M, (3, 16, 29))
    np.linalg.cholesky(P)                                    # SPD, every filter
    idx = np.unique(np.r_[0:4, np.random.default_rng(132).choice(np.arange(4, B - 4), 8, replace=False), B - 4:B])
    assert len(idx) == 16
    st, om, oP = oracle_step_batch(s, idx, nfk, nfkl, steps)
    assert st == 0
    for j, b in enumerate(idx):
        assert rel(P[b], oP[j]) <= TOL, b
        assert mean_err(lay, M[b], om[j]) <= TOL, b


# ------------------------------------------------------------------ 3. Tier B
def test_usckf_large_tier_b(slk):
    """N = 120: predict_sigma_points + slk_predict_from_sigma and update_functor (EXTERNAL Z) == the registered models;
    slk_update_innovation's S and innovation == numpy on the sigma points slk_update_sigma_points emits (meanSigmaPoints,
    covSigmaPoints + R, Usckf.hpp:280-282, :632-690), and the filter is untouched by both emissions."""
    nfk, nfkl, B = 12, 72, 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED6000)
    routes._usckf_functor_path(slk, s, nfk, nfkl, B)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    X = f.update_sigma_points()
    assert X.shape == (B, 2 * s["N"] + 1, s["Nq"])
    m = nfk
    SI = np.empty((B, m * m + m))
    z = np.ascontiguousarray(s["z"])
    Rc = np.ascontiguousarray(s["R"].T)
    lib = slk.load_library()
    assert lib.slk_update_innovation(f._h, slk.MM_VO_RELATIVE, None, 0, None, z.ctypes.data, m, Rc.ctypes.data, 0,
                                     SI.ctypes.data, slk.HOST) == 0
    assert (f.status() == 0).all()
    np.testing.assert_array_equal(f.PkAugmentedState(), s["P"])
    np.testing.assert_array_equal(f.muState(), s["mean"])
    for b in range(B):
        Z = np.array([npc.mm_vo_relative(x, nfk) for x in X[b]])
        zbar = Z.mean(axis=0)
        D = Z - zbar
        S = 0.5 * D.T @ D + s["R"]
        Sg = SI[b, :m * m].reshape(m, m).T
        assert rel(Sg, S) <= 1e-12, b
        assert np.abs(SI[b, m * m:] - (s["z"][b] - zbar)).max() <= 1e-12 * max(1.0, np.abs(s["z"][b]).max()), b


# ------------------------------------------------------------------ 4. bookkeeping across N = 96
def test_usckf_set_measurement_and_cloning_across_96(slk):
    """setMeasurement grows N 90 -> 110 (STATEK_L), a step, cloning in both modes, a step, setMeasurement back to N = 88
    and a step on the LDS kernels; every call against the oracle, status bits included (cloning(STATEK_I) leaves a
    singular covariance)."""
    B, nfk, nfkl = 3, 12, 42
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED7000)
    rng = np.random.default_rng(110)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    refs = [ref_usckf(s, b, nfk, nfkl) for b in range(B)]

    def compare(what, expect=None):
        P, M = f.PkAugmentedState(), f.muState()
        assert P.shape[1] == refs[0].N, what
        for b, r in enumerate(refs):
            eP, eM = expect[b] if expect else (r.P, r.mean)
            assert rel(P[b], eP) <= TOL and mean_err(r.lay, M[b], eM) <= TOL, (what, b)

    def step(what):
        f.clear_status()
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
        st = f.status()
        expect = []
        for b, r in enumerate(refs):
            sp = r.predict(pm_cv(s["u"][b]), s["Q"])
            Pp, Mp = r.P, r.mean
            su, acc = r.update(s["z"][b], o.mm_vo_relative(), s["R"])
            assert st[b] == (sp | su), (what, b, st[b], sp, su)
            # a failed factorisation leaves the filter as the predict left it (the oracle carries on with the partial
            # factor: its own state after such an update is not a reference)
            expect.append((Pp, Mp) if su & o.LLT_FAIL else (r.P, r.mean))
        compare(what, expect)

    def set_measurement(mode, n):
        zs = rng.uniform(1, 4, n)
        Rs = sc.dense_noise(n, scale=0.01, seed=n)
        f.setMeasurement(mode, zs, Rs)
        for r in refs:
            r.set_measurement(mode, zs, Rs)
        compare(("setMeasurement", mode, n))

    set_measurement(slk.STATEK_L, 62)
    assert f.N == 110
    step("step at N = 110")
    for mode in (slk.STATEK_L, slk.STATEK_I):
        f.cloning(mode)
        for r in refs:
            r.cloning(mode)
        compare(("cloning", mode))
    step("step after cloning")
    set_measurement(slk.STATEK_L, 40)
    assert f.N == 88
    step("step at N = 88")


# ------------------------------------------------------------------ 5. failure semantics
def test_usckf_large_failure_semantics(slk):
    """N = 132: an indefinite covariance raises SLK_ST_LLT_FAIL for that filter alone and leaves it bit-identical, its
    neighbours match the oracle; pose index 3 in device-resident parameters raises SLK_ST_BAD_INDEX."""
    import torch
    nfk, nfkl, B = 24, 72, 4
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED8000)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    P0 = s["P"].copy()
    P0[2, 50, 50] = -0.01
    f = slk.Usckf(mean=s["mean"], P=P0, nfk=nfk, nfkl=nfkl)
    f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    st = f.status()
    assert st[2] == slk.ST_LLT_FAIL and (np.delete(st, 2) == 0).all(), st
    P, M = f.PkAugmentedState(), f.muState()
    np.testing.assert_array_equal(P[2], P0[2])
    np.testing.assert_array_equal(M[2], s["mean"][2])
    for b in (0, 1, 3):
        r = ref_usckf(s, b, nfk, nfkl)
        stc, acc = r.update(s["z"][b], o.mm_vo_relative(), s["R"])
        assert stc == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b
    # device-resident pose index out of 0..2: the kernel reports it and skips the filter's update
    g = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    dev = torch.device("cuda", 0)
    params = np.array([[0.0], [1.0], [3.0], [2.0]])
    z = s["mean"][:, 0:3] + 0.01
    d = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in
         (("p", params), ("z", z), ("R", 0.01 * np.eye(3)))}
    g.update(d["z"], slk.MM_POSE_POSITION, d["p"], d["R"], gate=0)
    st = g.status()
    assert st[2] == slk.ST_BAD_INDEX and (np.delete(st, 2) == 0).all(), st
    np.testing.assert_array_equal(g.PkAugmentedState()[2], s["P"][2])
    np.testing.assert_array_equal(g.muState()[2], s["mean"][2])
    P, M = g.PkAugmentedState(), g.muState()
    for b in (0, 1, 3):
        r = ref_usckf(s, b, nfk, nfkl)
        stc, acc = r.update(z[b], o.mm_pose_position(int(params[b, 0])), 0.01 * np.eye(3))
        assert stc == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


# ------------------------------------------------------------------ 6. noise layouts
def test_usckf_large_noise_layouts(slk):
    """N = 108: per-filter copies of a shared R and Q, and a shared 1-D u against the same row tiled over the batch, give
    bit-identical results."""
    nfk, nfkl, B = 12, 60, 4
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EED9000)
    Q = sc.dense_noise(12, scale=0.001, seed=12)
    R = sc.dense_noise(nfk, scale=0.01, seed=nfk)
    u = s["u"][0]

    def run(u_, Q_, R_):
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
        f.step(slk.PM_CONST_VELOCITY, u_, Q_, s["z"], slk.MM_VO_RELATIVE, None, R_)
        f.step(slk.PM_CONST_VELOCITY, u_, Q_, s["z"], slk.MM_VO_RELATIVE, None, R_)
        assert (f.status() == 0).all()
        return f.PkAugmentedState(), f.muState()

    Pa, Ma = run(u, Q, R)
    Pb, Mb = run(np.tile(u, (B, 1)), np.tile(Q, (B, 1, 1)), np.tile(R, (B, 1, 1)))
    np.testing.assert_array_equal(Pa, Pb)
    np.testing.assert_array_equal(Ma, Mb)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        for _ in range(2):
            assert r.predict(pm_cv(u), Q) == 0
            st, acc = r.update(s["z"][b], o.mm_vo_relative(), R)
            assert st == 0 and acc == 1
        assert rel(Pa[b], r.P) <= TOL and mean_err(lay, Ma[b], r.mean) <= TOL, b


# ------------------------------------------------------------------ 7. C++ facade
def test_usckf_large_window_through_cpp_facade(slk):
    """tests/cpp/usckf_large_window.cpp: the facade Usckf at N = 90, setMeasurement(STATEK_L) to N = 120, predict and update
    with opaque functors -- the same calls through the Python package give the same covariance and mean."""
    import __graft_entry__ as ge
    ge.build()
    import facade_build
    res = facade_build.run(name="usckf_large_window")
    nfk, nfkl = 12, 42
    P0, m0 = res["large_ctor_P"], res["large_ctor_mean"][:, 0]
    f = slk.Usckf(mean=m0[None], P=P0[None], nfk=nfk, nfkl=nfkl)
    zl = 1.5 + 0.01 * np.arange(72)
    f.setMeasurement(slk.STATEK_L, zl, 0.008 * np.eye(72))
    assert f.N == 120

    def drift(x):
        y = np.array(x, dtype=np.float64)
        y[0:3] = x[0:3] + 0.01 * x[7:10]
        return y
    f.predict_functor(drift, 0.001 * np.eye(12))
    lay = o.layout(o.AUGMENTED, 0, nfk, 72)
    assert rel(f.PkAugmentedState()[0], res["large_pred_P"]) <= TOL
    assert mean_err(lay, f.muState()[0], res["large_pred_mean"][:, 0]) <= TOL
    f.update_functor(np.array([0.55, -0.28, 1.02, 1.48]), lambda x: np.r_[x[0:3], x[39 + nfk]], 0.01 * np.eye(4))
    assert int(res["large_status"][0, 0]) == 0 and (f.status() == 0).all()
    assert rel(f.PkAugmentedState()[0], res["large_upd_P"]) <= TOL
    assert mean_err(lay, f.muState()[0], res["large_upd_mean"][:, 0]) <= TOL
