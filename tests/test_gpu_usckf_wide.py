"""Usckf updates with more than MAXM = 32 measurement rows (csrc/slk_usckf_wide.hpp, launch_usckf_wide in
csrc/slk_api.hip), at every state size, against the fp64 CPU oracle with the helpers and the tolerance of
test_gpu_routes.py.  Every case here except the Msckf scope guard was refused with SlkError before that path existed.
Run with `pytest -m gpu` on an MI355X.
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

# SLK_MM_VO_RELATIVE takes m = nfk rows: every shape here has nfk > MAXM
VO_SHAPES = [(33, 0), (36, 24), (48, 12), (60, 0), (36, 60), (48, 100), (90, 30)]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def features(s, nfeat, seed):
    """nfeat MM_FEATURE_PROJ features seen round-robin from poses 0, 1, 2 -> (feat [B, nfeat, 4], z [B, 2 nfeat])."""
    return sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(nfeat)), seed=seed)


# ------------------------------------------------------------------ 1. VO_RELATIVE, m = nfk > 32
@pytest.mark.parametrize("nfk,nfkl", VO_SHAPES, ids=[f"N{36 + a + b}-nfk{a}-nfkl{b}" for a, b in VO_SHAPES])
def test_usckf_wide_vo_sweep(slk, nfk, nfkl):
    """predict alone, update alone, fused step with MM_VO_RELATIVE at m = nfk; the whole-vector gate with nfk > 9 degrees
    of freedom rejects every filter and leaves it bit-identical with SLK_ST_ALL_REJECTED."""
    B = 4
    N = 36 + nfk + nfkl
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEDA000 + N)
    routes._usckf_vo_chain(slk, s, nfk, nfkl, B)
    routes._usckf_vo_gated(slk, s, nfk, nfkl, B)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"], gate=nfk)
    assert (f.status() == slk.ST_ALL_REJECTED).all() and (f.outliers() == 1).all()
    np.testing.assert_array_equal(f.PkAugmentedState(), s["P"])
    np.testing.assert_array_equal(f.muState(), s["mean"])


# ------------------------------------------------------------------ 2. FEATURE_PROJ, m = 34 / 64 / 128
@pytest.mark.parametrize("nfk,nfkl", [(3, 9), (12, 48), (30, 98)], ids=["N48", "N96", "N164"])
@pytest.mark.parametrize("nfeat", [17, 32, 64], ids=["m34", "m64", "m128"])
def test_usckf_wide_feature_proj(slk, nfk, nfkl, nfeat):
    """MM_FEATURE_PROJ with 2 nfeat rows, fused with a predict (at N = 48 the unit shape: the predict leaves the lower
    triangle only, which the wide update reads), then an update alone."""
    B = 3
    N = 36 + nfk + nfkl
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEDB000 + N + nfeat)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    feat, z = features(s, nfeat, seed=N + nfeat)
    m = 2 * nfeat
    R = 0.01 * np.eye(m)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], z, slk.MM_FEATURE_PROJ, feat, R)
    f.update(z, slk.MM_FEATURE_PROJ, feat, R)
    assert (f.status() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    routes.check_batch_properties(P, M, (3, 16, 29))
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
        for _ in range(2):
            st, acc = r.update(z[b], o.mm_feature_proj(feat[b]), R)
            assert st == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


# ------------------------------------------------------------------ 3. step == predict + update
@pytest.mark.parametrize("nfk,nfkl", [(3, 9), (36, 8), (36, 60)], ids=["N48-split", "N80-fused", "N132-general"])
def test_usckf_wide_step_equals_predict_update(slk, nfk, nfkl):
    """At m = 34 the predict half of a step takes the predict-only route of its N and the wide update follows as a launch
    of its own: bit-identical to predict followed by update."""
    B = 4
    N = 36 + nfk + nfkl
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEDC000 + N)
    feat, z = features(s, 17, seed=N)
    R = sc.dense_noise(34, scale=0.01, seed=N)
    a = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    b = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    for _ in range(2):
        a.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], z, slk.MM_FEATURE_PROJ, feat, R)
        b.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"])
        b.update(z, slk.MM_FEATURE_PROJ, feat, R)
    assert (a.status() == 0).all() and (b.status() == 0).all()
    np.testing.assert_array_equal(a.PkAugmentedState(), b.PkAugmentedState())
    np.testing.assert_array_equal(a.muState(), b.muState())
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    P, M = a.PkAugmentedState(), a.muState()
    for i in range(B):
        r = ref_usckf(s, i, nfk, nfkl)
        for _ in range(2):
            assert r.predict(pm_cv(s["u"][i]), s["Q"]) == 0
            st, acc = r.update(z[i], o.mm_feature_proj(feat[i]), R)
            assert st == 0 and acc == 1
        assert rel(P[i], r.P) <= TOL and mean_err(lay, M[i], r.mean) <= TOL, i


# ------------------------------------------------------------------ 4. Tier B
def test_usckf_wide_tier_b(slk):
    """N = 96, m = 48: update_functor (slk_update_from_sigma, EXTERNAL Z) == the registered model; slk_update_innovation's
    S and innovation == numpy on the emitted sigma points, and the filter is untouched."""
    nfk, nfkl, B = 48, 12, 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEDD000)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    a = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    b = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    a.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    b.update_functor(s["z"], lambda x: npc.mm_vo_relative(x, nfk), s["R"])
    assert (a.status() == 0).all() and (b.status() == 0).all()
    Pa, Pb, Ma, Mb = a.PkAugmentedState(), b.PkAugmentedState(), a.muState(), b.muState()
    for i in range(B):
        assert rel(Pb[i], Pa[i]) <= 1e-12 and mean_err(lay, Mb[i], Ma[i]) <= 1e-12, i

    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    X = f.update_sigma_points()
    m = nfk
    SI = np.empty((B, m * m + m))
    z = np.ascontiguousarray(s["z"])
    R = sc.dense_noise(m, scale=0.01, seed=m)
    Rc = np.ascontiguousarray(R.T)
    lib = slk.load_library()
    assert lib.slk_update_innovation(f._h, slk.MM_VO_RELATIVE, None, 0, None, z.ctypes.data, m, Rc.ctypes.data, 0,
                                     SI.ctypes.data, slk.HOST) == 0
    assert (f.status() == 0).all()
    np.testing.assert_array_equal(f.PkAugmentedState(), s["P"])
    np.testing.assert_array_equal(f.muState(), s["mean"])
    for i in range(B):
        Z = np.array([npc.mm_vo_relative(x, nfk) for x in X[i]])
        zbar = Z.mean(axis=0)
        D = Z - zbar
        S = 0.5 * D.T @ D + R
        Sg = SI[i, :m * m].reshape(m, m).T
        assert rel(Sg, S) <= 1e-12, i
        assert np.abs(SI[i, m * m:] - (s["z"][i] - zbar)).max() <= 1e-12 * max(1.0, np.abs(s["z"][i]).max()), i


# ------------------------------------------------------------------ 5. full batch
def test_usckf_wide_full_batch(slk):
    """N = 96, m = 48, B = 1024, three fused steps: status 0, exactly symmetric SPD covariances, unit quaternions, 16
    sampled filters against the oracle."""
    nfk, nfkl, B, steps = 48, 12, 1024, 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEDE000)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    for _ in range(steps):
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    routes.check_batch_properties(P, M, (3, 16, 29))
    idx = np.unique(np.r_[0:4, np.random.default_rng(96).choice(np.arange(4, B - 4), 8, replace=False), B - 4:B])
    assert len(idx) == 16
    N = s["N"]
    om = np.ascontiguousarray(s["mean"][idx])
    oP = np.ascontiguousarray(np.transpose(s["P"][idx], (0, 2, 1))).reshape(len(idx), -1)
    st = o.usckf_step_batch(nfk, nfkl, steps, om, oP, np.ascontiguousarray(s["u"][idx]),
                            np.ascontiguousarray(s["z"][idx]), s["Q"], s["R"])
    assert st == 0
    oP = routes.colmajor_P(oP, N)
    for j, b in enumerate(idx):
        assert rel(P[b], oP[j]) <= TOL, b
        assert mean_err(lay, M[b], om[j]) <= TOL, b


# ------------------------------------------------------------------ 6. noise layouts
def test_usckf_wide_noise_layouts(slk):
    """N = 96, m = 48: a dense correlated R per filter (r_stride = m * m) == the same R shared, bit for bit."""
    nfk, nfkl, B = 48, 12, 4
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEDF000)
    R = sc.dense_noise(nfk, scale=0.01, seed=nfk)

    def run(R_):
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
        for _ in range(2):
            f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, R_)
        assert (f.status() == 0).all()
        return f.PkAugmentedState(), f.muState()

    Pa, Ma = run(R)
    Pb, Mb = run(np.tile(R, (B, 1, 1)))
    np.testing.assert_array_equal(Pa, Pb)
    np.testing.assert_array_equal(Ma, Mb)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    for b in range(B):
        r = ref_usckf(s, b, nfk, nfkl)
        for _ in range(2):
            assert r.predict(pm_cv(s["u"][b]), s["Q"]) == 0
            st, acc = r.update(s["z"][b], o.mm_vo_relative(), R)
            assert st == 0 and acc == 1
        assert rel(Pa[b], r.P) <= TOL and mean_err(lay, Ma[b], r.mean) <= TOL, b


# ------------------------------------------------------------------ 7. failure semantics
def _neighbours_match(P, M, s, z, model, R, nfk, nfkl, skip, lay):
    for b in range(s["B"]):
        if b == skip:
            continue
        r = ref_usckf(s, b, nfk, nfkl)
        st, acc = r.update(z[b], model(b), R[b] if R.ndim == 3 else R)
        assert st == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


def test_usckf_wide_failure_semantics(slk):
    """N = 96, m = 48: an indefinite P gives SLK_ST_LLT_FAIL, an R that makes S indefinite SLK_ST_SINGULAR, pose index 3
    in device-resident FEATURE_PROJ parameters (m = 34) SLK_ST_BAD_INDEX; the filter concerned stays bit-identical, its
    neighbours match the oracle."""
    import torch
    nfk, nfkl, B = 48, 12, 4
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEE0000)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    vo = lambda b: o.mm_vo_relative()  # noqa: E731

    P0 = s["P"].copy()
    P0[2, 50, 50] = -0.01
    f = slk.Usckf(mean=s["mean"], P=P0, nfk=nfk, nfkl=nfkl)
    f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    st = f.status()
    assert st[2] == slk.ST_LLT_FAIL and (np.delete(st, 2) == 0).all(), st
    P, M = f.PkAugmentedState(), f.muState()
    np.testing.assert_array_equal(P[2], P0[2])
    np.testing.assert_array_equal(M[2], s["mean"][2])
    _neighbours_match(P, M, s, s["z"], vo, s["R"], nfk, nfkl, 2, lay)

    Rb = np.tile(s["R"], (B, 1, 1))
    Rb[1] = -10.0 * np.eye(nfk)
    g = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    g.update(s["z"], slk.MM_VO_RELATIVE, None, Rb)
    st = g.status()
    assert st[1] == slk.ST_SINGULAR and (np.delete(st, 1) == 0).all(), st
    P, M = g.PkAugmentedState(), g.muState()
    np.testing.assert_array_equal(P[1], s["P"][1])
    np.testing.assert_array_equal(M[1], s["mean"][1])
    _neighbours_match(P, M, s, s["z"], vo, Rb, nfk, nfkl, 1, lay)

    feat, z = features(s, 17, seed=3)
    feat[3, 5, 3] = 3.0
    R = 0.01 * np.eye(34)
    h = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    dev = torch.device("cuda", 0)
    d = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in
         (("p", feat.reshape(B, -1)), ("z", z), ("R", R))}
    h.update(d["z"], slk.MM_FEATURE_PROJ, d["p"], d["R"])
    st = h.status()
    assert st[3] == slk.ST_BAD_INDEX and (np.delete(st, 3) == 0).all(), st
    P, M = h.PkAugmentedState(), h.muState()
    np.testing.assert_array_equal(P[3], s["P"][3])
    np.testing.assert_array_equal(M[3], s["mean"][3])
    _neighbours_match(P, M, s, z, lambda b: o.mm_feature_proj(feat[b]), R, nfk, nfkl, 3, lay)


# ------------------------------------------------------------------ 8. setMeasurement across the old limit
def test_usckf_wide_set_measurement_across_32(slk):
    """setMeasurement(STATEK) grows featuresk 30 -> 36 (N = 66 -> 72), then a VO update with the new 36 rows.  (No
    featuresk_l: with them, STATEK mode reads their old block at the new offset, Usckf.hpp:338-342, and the covariance it
    leaves is singular on both sides.)"""
    B, nfk, nfkl = 3, 30, 0
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x5EEE1000)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    refs = [ref_usckf(s, b, nfk, nfkl) for b in range(B)]
    zs = np.random.default_rng(36).uniform(1, 4, 36)
    Rs = sc.dense_noise(36, scale=0.01, seed=36)
    f.setMeasurement(slk.STATEK, zs, Rs)
    for r in refs:
        r.set_measurement(slk.STATEK, zs, Rs)
    assert f.N == 72
    lay = o.layout(o.AUGMENTED, 0, 36, nfkl)
    z = np.array([npc.mm_vo_relative(x, 36) for x in f.muState()]) + 0.02
    R = 0.01 * np.eye(36)
    f.update(z, slk.MM_VO_RELATIVE, None, R)
    assert (f.status() == 0).all()
    P, M = f.PkAugmentedState(), f.muState()
    for b, r in enumerate(refs):
        st, acc = r.update(z[b], o.mm_vo_relative(), R)
        assert st == 0 and acc == 1
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, b


# ------------------------------------------------------------------ 9. scope guard: Msckf keeps its limit
def test_usckf_wide_msckf_keeps_row_limit(slk):
    """Msckf update with m = 34 rows is still refused before any launch; the filter is left unmodified."""
    B, k = 2, 4
    s = sc.synthetic_msckf(B, k)
    feat, z = sc.msckf_features(s["mean"], k, 17, np.random.default_rng(34))
    f = slk.Msckf(mean=s["mean"], P=s["P"])
    with pytest.raises(slk.SlkError):
        f.update(z, slk.MM_FEATURE_PROJ, feat, 0.01 * np.eye(34))
    np.testing.assert_array_equal(f.getPk(), s["P"])
    np.testing.assert_array_equal(f.muState(), s["mean"])
    assert (f.status() == 0).all()


# ------------------------------------------------------------------ 10. C++ facade
def test_usckf_wide_update_through_cpp_facade(slk):
    """tests/cpp/usckf_wide_update.cpp: the facade Usckf (no featuresk_l) grows featuresk 30 -> 36 by setMeasurement, predicts and updates
    with VoRelativeModel over 36 rows -- the same calls through the Python package give the same covariance and mean."""
    import __graft_entry__ as ge
    ge.build()
    import facade_build
    res = facade_build.run(name="usckf_wide_update")
    nfk, nfkl = 30, 0
    P0, m0 = res["wide_ctor_P"], res["wide_ctor_mean"][:, 0]
    f = slk.Usckf(mean=m0[None], P=P0[None], nfk=nfk, nfkl=nfkl)
    zk = 2.5 + 0.01 * np.arange(36)
    f.setMeasurement(slk.STATEK, zk, 0.008 * np.eye(36))
    assert f.N == 72
    u = np.array([[1.0, 0.2, -0.1, 0.01, -0.02, 0.03, 0.01]])
    f.predict(slk.PM_CONST_VELOCITY, u, 0.001 * np.eye(12))
    lay = o.layout(o.AUGMENTED, 0, 36, nfkl)
    assert rel(f.PkAugmentedState()[0], res["wide_pred_P"]) <= 1e-12
    assert mean_err(lay, f.muState()[0], res["wide_pred_mean"][:, 0]) <= 1e-12
    z = res["wide_z"][:, 0]
    f.update(z[None], slk.MM_VO_RELATIVE, None, 0.01 * np.eye(36), gate=0)
    assert int(res["wide_status"][0, 0]) == 0 and (f.status() == 0).all()
    assert rel(f.PkAugmentedState()[0], res["wide_upd_P"]) <= 1e-12
    assert mean_err(lay, f.muState()[0], res["wide_upd_mean"][:, 0]) <= 1e-12
    r = o.Usckf(nfk=nfk, nfkl=nfkl, mean=m0, P=P0)
    r.set_measurement(slk.STATEK, zk, 0.008 * np.eye(36))
    assert r.predict(pm_cv(u[0]), 0.001 * np.eye(12)) == 0
    st, acc = r.update(z, o.mm_vo_relative(), 0.01 * np.eye(36))
    assert st == 0 and acc == 1
    assert rel(res["wide_upd_P"], r.P) <= TOL and mean_err(lay, res["wide_upd_mean"][:, 0], r.mean) <= TOL
