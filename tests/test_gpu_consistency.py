"""NEES and Gaussian state draws on the device (slk_nees / slk_sample_states, csrc/slk_consistency.hpp) against numpy
(np.linalg.cholesky / solve) and the CPU oracle's manifold operators (oracle.boxminus / oracle.boxplus).  Every case here
fails without the two calls.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc

pytestmark = pytest.mark.gpu

MSCKF_K = [0, 1, 8, 31, 35]                       # N = 12, 18, 60, 198, 222
USCKF_SHAPES = [(3, 9), (12, 48), (30, 98)]       # N = 48, 96, 164


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def perturbed_truth(lay, mean, rng, scale=0.05, negate=None):
    """truth = mean [+] d for a random tangent d; negate = filter index whose first quaternion is negated (same rotation,
    w < 0)"""
    B = mean.shape[0]
    N = o.dof(lay)
    t = np.stack([o.boxplus(lay, mean[b], rng.normal(0, scale, N)) for b in range(B)])
    if negate is not None:
        t[negate, 3:7] *= -1.0
    return t


def ranges(N, kind):
    r = [(0, N), (0, 12), (0, 6), (3, 3), (4, 7)]                 # full, state, pose, attitude, one starting inside a rotation
    r.append((N - 6, 6) if kind == o.MULTI else (24, 12))         # the last clone / statek_i
    return r


def ref_nees(lay, mean, P, truth, t0, n):
    B = mean.shape[0]
    e = np.stack([o.boxminus(lay, truth[b], mean[b])[t0:t0 + n] for b in range(B)])
    Ps = P[:, t0:t0 + n, t0:t0 + n]
    nees = np.array([e[b] @ np.linalg.solve(Ps[b], e[b]) for b in range(B)])
    return nees, e


def check_ranges(slk, f, lay, mean, P, truth):
    N = o.dof(lay)
    for t0, n in ranges(N, lay.kind):
        ne, err = f.nees(truth, t0, n, error=True)
        rn, re = ref_nees(lay, mean, P, truth, t0, n)
        assert err.shape == (mean.shape[0], n)
        np.testing.assert_allclose(err, re, rtol=0, atol=1e-12, err_msg=f"e on [{t0}, {t0 + n})")
        np.testing.assert_allclose(ne, rn, rtol=1e-9, atol=0, err_msg=f"NEES on [{t0}, {t0 + n})")


# ------------------------------------------------------------------ 1. NEES on every shape and range
@pytest.mark.parametrize("k", MSCKF_K, ids=[f"N{12 + 6 * k}" for k in MSCKF_K])
def test_msckf_nees_ranges(slk, k):
    B = 3
    s = sc.synthetic_msckf(B, k, seed=0xC0115 + k)
    lay = o.layout(o.MULTI, k)
    truth = perturbed_truth(lay, s["mean"], np.random.default_rng(k), negate=1)
    f = slk.Msckf(s["mean"], s["P"])
    check_ranges(slk, f, lay, s["mean"], s["P"], truth)


@pytest.mark.parametrize("nfk,nfkl", USCKF_SHAPES, ids=[f"N{36 + a + b}" for a, b in USCKF_SHAPES])
def test_usckf_nees_ranges(slk, nfk, nfkl):
    B = 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0xC0116 + nfk)
    lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
    truth = perturbed_truth(lay, s["mean"], np.random.default_rng(nfk), negate=2)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    check_ranges(slk, f, lay, s["mean"], s["P"], truth)


# ------------------------------------------------------------------ 2. draws and the round trip
def check_samples(slk, f, lay, mean, P, S, seed):
    B, N = mean.shape[0], o.dof(lay)
    nz = np.random.default_rng(seed).normal(0, 1, (B, S, N))
    X = f.sample_states(nz)
    assert X.shape == (B, S, o.storage(lay))
    for b in range(B):
        L = np.linalg.cholesky(P[b])
        for s in (0, S // 2, S - 1):
            np.testing.assert_allclose(X[b, s], o.boxplus(lay, mean[b], L @ nz[b, s]), rtol=1e-12, atol=1e-12)
    # round trip: the NEES of a draw is |n|^2
    for s in (0, S - 1):
        ne = f.nees(X[:, s, :])
        np.testing.assert_allclose(ne, (nz[:, s, :] ** 2).sum(axis=1), rtol=1e-9, atol=0)


@pytest.mark.parametrize("k", MSCKF_K, ids=[f"N{12 + 6 * k}" for k in MSCKF_K])
@pytest.mark.parametrize("S", [1, 17])
def test_msckf_sample_states(slk, k, S):
    B = 2
    s = sc.synthetic_msckf(B, k, seed=0xD4A3 + k)
    f = slk.Msckf(s["mean"], s["P"])
    check_samples(slk, f, o.layout(o.MULTI, k), s["mean"], s["P"], S, seed=k + S)


@pytest.mark.parametrize("nfk,nfkl", USCKF_SHAPES, ids=[f"N{36 + a + b}" for a, b in USCKF_SHAPES])
def test_usckf_sample_states(slk, nfk, nfkl):
    B = 2
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0xD4A4 + nfk)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    check_samples(slk, f, o.layout(o.AUGMENTED, 0, nfk, nfkl), s["mean"], s["P"], 33, seed=nfk)


# ------------------------------------------------------------------ 3. the strict upper triangle is never read
@pytest.mark.parametrize("k", [1, 8, 31], ids=["N18", "N60", "N198"])
def test_nan_upper_triangle(slk, k):
    B = 2
    s = sc.synthetic_msckf(B, k, seed=0x0FFD + k)
    lay = o.layout(o.MULTI, k)
    N = s["N"]
    Pn = s["P"].copy()
    iu = np.triu_indices(N, 1)
    Pn[:, iu[0], iu[1]] = np.nan
    f = slk.Msckf(s["mean"], s["P"])
    f.set_state(None, Pn)
    truth = perturbed_truth(lay, s["mean"], np.random.default_rng(7))
    ne = f.nees(truth)
    assert np.isfinite(ne).all()
    rn, _ = ref_nees(lay, s["mean"], s["P"], truth, 0, N)
    np.testing.assert_allclose(ne, rn, rtol=1e-9)
    nz = np.random.default_rng(8).normal(0, 1, (B, 4, N))
    X = f.sample_states(nz)
    L = np.linalg.cholesky(s["P"][0])
    np.testing.assert_allclose(X[0, 3], o.boxplus(lay, s["mean"][0], L @ nz[0, 3]), rtol=1e-12, atol=1e-12)


def test_after_exact_shape_steps(slk):
    """k = 8, m = 8 fused steps leave the strict upper triangle stale on the device: the calls read the lower one."""
    B, k, m = 16, 8, 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0x57A1E)
    f = slk.Msckf(s["mean"], s["P"])
    for _ in range(2):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    lay = o.layout(o.MULTI, k)
    truth = perturbed_truth(lay, s["mean"], np.random.default_rng(9))
    nz = np.random.default_rng(10).normal(0, 1, (B, 2, s["N"]))
    ne_full, ne_pose = f.nees(truth), f.nees(truth, 0, 6)
    X = f.sample_states(nz)
    P, mu = f.getPk(), f.muState()                 # (mirrors the upper triangle: after the calls)
    np.testing.assert_allclose(ne_full, ref_nees(lay, mu, P, truth, 0, s["N"])[0], rtol=1e-9)
    np.testing.assert_allclose(ne_pose, ref_nees(lay, mu, P, truth, 0, 6)[0], rtol=1e-9)
    for b in (0, B - 1):
        np.testing.assert_allclose(X[b, 1], o.boxplus(lay, mu[b], np.linalg.cholesky(P[b]) @ nz[b, 1]), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ 4. a block that is not positive definite
@pytest.mark.parametrize("kind", ["msckf", "usckf"])
def test_non_pd_filter_gets_nan(slk, kind):
    B = 4
    if kind == "msckf":
        s = sc.synthetic_msckf(B, 8, seed=0xBAD)
        lay = o.layout(o.MULTI, 8)
        f = slk.Msckf(s["mean"], s["P"])
    else:
        s = sc.synthetic_usckf(B, nfk=3, nfkl=9, seed=0xBAD)
        lay = o.layout(o.AUGMENTED, 0, 3, 9)
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
    N = s["N"]
    P = s["P"].copy()
    P[1, 7, 7] = -1.0                              # filter 1: not PD on any range containing index 7
    P[2, 40, 40] = np.nan                          # filter 2: NaN pivot
    f.setPk(P) if kind == "msckf" else f.set_state(None, P)
    f.clear_status()
    truth = perturbed_truth(lay, s["mean"], np.random.default_rng(11))
    before = (f.muState(), f._getP(), f.status(), f.outliers())
    ne = f.nees(truth)
    assert np.isnan(ne[1]) and np.isnan(ne[2]) and np.isfinite(ne[[0, 3]]).all()
    rn, _ = ref_nees(lay, s["mean"], P, truth, 0, N)
    np.testing.assert_allclose(ne[[0, 3]], rn[[0, 3]], rtol=1e-9)
    ne6 = f.nees(truth, 0, 6)                      # the pose block of every filter is still PD
    np.testing.assert_allclose(ne6, ref_nees(lay, s["mean"], P, truth, 0, 6)[0], rtol=1e-9)
    X = f.sample_states(np.random.default_rng(12).normal(0, 1, (B, 5, N)))
    assert np.isnan(X[1]).all() and np.isnan(X[2]).all() and np.isfinite(X[[0, 3]]).all()
    after = (f.muState(), f._getP(), f.status(), f.outliers())
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert (after[2] == 0).all()


# ------------------------------------------------------------------ 5. a full batch, device tensors, invalid input
def test_batch_4096_n60(slk):
    B, k = 4096, 8
    s = sc.synthetic_msckf(B, k, seed=0xB4096)
    lay = o.layout(o.MULTI, k)
    rng = np.random.default_rng(13)
    truth = s["mean"].copy()
    truth[:, 0:3] += rng.normal(0, 0.05, (B, 3))
    truth[:, 13:16] += rng.normal(0, 0.05, (B, 3))
    f = slk.Msckf(s["mean"], s["P"])
    ne, err = f.nees(truth, error=True)
    pick = rng.choice(B, 64, replace=False)
    rn, re = ref_nees(lay, s["mean"][pick], s["P"][pick], truth[pick], 0, s["N"])
    np.testing.assert_allclose(ne[pick], rn, rtol=1e-9)
    np.testing.assert_allclose(err[pick], re, rtol=0, atol=1e-12)
    # vectorised check of every filter: the errors are exact differences here, NEES = e^T P^-1 e
    e_all = truth[:, :3] - s["mean"][:, :3]
    assert np.abs(err[:, :3] - e_all).max() < 1e-12
    full = np.einsum("bi,bi->b", err, np.linalg.solve(s["P"], err[..., None])[..., 0])
    np.testing.assert_allclose(ne, full, rtol=1e-9)


def test_torch_device_tensors(slk):
    import torch
    dev = torch.device("cuda", 0)
    B, k = 64, 8
    s = sc.synthetic_msckf(B, k, seed=0x7041)
    lay = o.layout(o.MULTI, k)
    truth = perturbed_truth(lay, s["mean"], np.random.default_rng(14))
    f = slk.Msckf(s["mean"], s["P"])
    tt = torch.from_numpy(truth).to(dev)
    ne, err = f.nees(tt, 3, 9, error=True)
    assert ne.is_cuda and err.is_cuda and tuple(err.shape) == (B, 9)
    ne_h, err_h = f.nees(truth, 3, 9, error=True)
    np.testing.assert_array_equal(ne.cpu().numpy(), ne_h)
    np.testing.assert_array_equal(err.cpu().numpy(), err_h)
    torch.manual_seed(0)
    nz = torch.randn((B, 64, s["N"]), dtype=torch.float64, device=dev)
    X = f.sample_states(nz)
    assert X.is_cuda and tuple(X.shape) == (B, 64, s["Nq"])
    np.testing.assert_array_equal(X.cpu().numpy(), f.sample_states(nz.cpu().numpy()))
    rt = f.nees(X[:, 63, :].contiguous())
    np.testing.assert_allclose(rt.cpu().numpy(), (nz[:, 63, :] ** 2).sum(dim=1).cpu().numpy(), rtol=1e-9)


def test_invalid_arguments(slk):
    B, k = 2, 1
    s = sc.synthetic_msckf(B, k, seed=0x1A7)
    f = slk.Msckf(s["mean"], s["P"])
    N, Nq = s["N"], s["Nq"]
    truth = s["mean"].copy()
    before = (f.muState(), f._getP())
    for t0, n in [(-1, 3), (0, 0), (0, -2), (N - 5, 6), (N, 1), (1, N)]:
        with pytest.raises(slk.SlkError, match="slk_nees failed with code -1"):
            f.nees(truth, t0, n)
    with pytest.raises(slk.SlkError, match="slk_nees failed with code -1"):
        f.nees(None)
    with pytest.raises(slk.SlkError, match="slk_sample_states failed with code -1"):
        f.sample_states(np.zeros((B, 0, N)))
    with pytest.raises(slk.SlkError, match="slk_sample_states failed with code -1"):
        f.sample_states(None)
    lib, h = f._lib, f._h
    t = np.ascontiguousarray(truth)
    out = np.empty(B)
    nz = np.zeros((B, 1, N))
    X = np.empty((B, 1, Nq))
    assert lib.slk_nees(h, t.ctypes.data, 0, N, None, None, slk.HOST) == slk.E_INVALID
    assert lib.slk_nees(h, None, 0, N, out.ctypes.data, None, slk.HOST) == slk.E_INVALID
    assert lib.slk_sample_states(h, nz.ctypes.data, 1, None, slk.HOST) == slk.E_INVALID
    assert lib.slk_sample_states(h, None, 1, X.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_sample_states(h, nz.ctypes.data, 0, X.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_nees(None, t.ctypes.data, 0, N, out.ctypes.data, None, slk.HOST) == slk.E_INVALID
    after = (f.muState(), f._getP())
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    assert (f.status() == 0).all()


# ------------------------------------------------------------------ 6. the C++ facade
def test_consistency_through_cpp_facade(slk):
    import facade_build
    res = facade_build.run(name="consistency_facade")
    for kind in ("msckf", "usckf"):
        mean, truth, P, nz = (res[f"{kind}_{n}"] for n in ("mean", "truth", "P", "noise"))
        mean, truth, nz = mean[:, 0][None], truth[:, 0][None], nz.T[None]
        if kind == "msckf":
            k = (mean.shape[1] - 13) // 7
            lay = o.layout(o.MULTI, k)
            f = slk.Msckf(mean, P[None])
            cases = {"full": (0, None), "att": (3, 3), "clone": (P.shape[0] - 6, 6)}
        else:
            nfk, nfkl = 3, mean.shape[1] - 39 - 3
            lay = o.layout(o.AUGMENTED, 0, nfk, nfkl)
            f = slk.Usckf(mean=mean, P=P[None], nfk=nfk, nfkl=nfkl)
            cases = {"full": (0, None), "pose": (0, 6)}
        for name, (t0, n) in cases.items():
            ne = f.nees(truth, t0, n)
            np.testing.assert_allclose(res[f"{kind}_nees_{name}"][0, 0], ne[0], rtol=1e-12)
            nn = P.shape[0] - t0 if n is None else n
            np.testing.assert_allclose(ne[0], ref_nees(lay, mean, P[None], truth, t0, nn)[0][0], rtol=1e-9)
        if kind == "msckf":
            _, err = f.nees(truth, 3, 3, error=True)
            np.testing.assert_array_equal(res["msckf_err_att"][:, 0], err[0])
        X = f.sample_states(nz)
        np.testing.assert_array_equal(res[f"{kind}_samples"].T, X[0])
        assert int(res[f"{kind}_size_checks"][0, 0]) == 3          # wrong noise rows and wrong truth shape both throw
    # a window grown through muState() + setPk right before the draw: drawn at the new N
    mean, P, nz = res["grown_mean"][:, 0][None], res["grown_P"], res["grown_noise"].T[None]
    f = slk.Msckf(mean, P[None])
    assert f.N == P.shape[0] == nz.shape[2]
    np.testing.assert_array_equal(res["grown_samples"].T, f.sample_states(nz)[0])
