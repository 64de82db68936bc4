"""slk_ensemble_moments on the device (csrc/slk_ensemble.hpp) against the numpy twin of tests/ensemble_ref.py: every shape,
G in {1, 8, B}, four kinds of weights, both modes, six ranges, host and device routes.  The tolerances are the derived
ones of ensemble_ref.check_against_twin.  Every case here fails without the call.  Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
import ensemble_ref as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def make_filter(slk, b, mean=None, P=None):
    mean, P = b["mean"] if mean is None else mean, b["P"] if P is None else P
    if b["kind"] == "msckf":
        return slk.Msckf(mean, P)
    return slk.Usckf(mean=mean, P=P, nfk=b["args"]["nfk"], nfkl=b["args"]["nfkl"])


def snapshot(f):
    return f.muState(), f._getP(), f.status(), f.outliers()


def same_bits(a, b, what=""):
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{what} {k}: not bit-identical"


def to_numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ------------------------------------------------------------------ 1. against the twin
@pytest.mark.parametrize("mode", ["error", "mixture"])
@pytest.mark.parametrize("gi", [0, 1, 2], ids=["G1", "G8", "GB"])
@pytest.mark.parametrize("name", er.SHAPE_IDS)
def test_moments_against_twin(slk, name, gi, mode):
    import torch
    dev = torch.device("cuda", 0)
    B = er.SHAPES[er.SHAPE_IDS.index(name)][3]
    G = er.group_counts(B)[gi]
    b = er.bank(name, G)
    lay = b["lay"]
    truth = er.truth_of(b) if mode == "error" else None
    f = make_filter(slk, b)
    before = snapshot(f)
    t_dev = torch.from_numpy(truth).to(dev) if truth is not None else None
    for wkind in er.WEIGHT_KINDS:
        w = er.weights_of(wkind, B, G)
        twin = er.Twin(lay, b["mean"], w, truth, G)
        w_dev = torch.from_numpy(w).to(dev) if w is not None else None
        for t0, n in er.ranges(lay):
            what = f"{name} G={G} {wkind} {mode} [{t0},{t0 + n})"
            got = f.ensemble_moments(w, truth, t0, n, groups=G, ess=True)
            ref = twin.moments(b["P"], t0, n)
            assert got["spread"].shape == (G, n, n) and got["center"].shape == ref["center"].shape, what
            er.check_against_twin(lay, got, ref, mode == "error", what)
            same_bits(got, f.ensemble_moments(w, truth, t0, n, groups=G, ess=True), what + " second call")
            gd = f.ensemble_moments(w_dev, t_dev, t0, n, groups=G, ess=True, device=dev)     # the device route
            assert all(v.is_cuda for v in gd.values())
            same_bits(got, to_numpy(gd), what + " device route")
    after = snapshot(f)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes(), name + ": the call changed the filter"


# ------------------------------------------------------------------ 2. twin-free checks
@pytest.mark.parametrize("name", ["msckf_n12", "msckf_n60", "usckf_n48"])
def test_identical_filters(slk, name):
    """spread is zero to 1e-24 absolute, mean_cov == P to 1e-14 relative"""
    b = er.bank(name, 1)
    B, N, lay = 1024, b["N"], b["lay"]
    mean, P = np.repeat(b["mean"][:1], B, axis=0), np.repeat(b["P"][:1], B, axis=0)
    truth = np.repeat(o.boxplus(lay, mean[0], np.random.default_rng(3).normal(0, 0.05, N))[None], B, axis=0)
    f = make_filter(slk, b, mean, P)
    w = np.random.default_rng(4).uniform(0.1, 1.0, B)
    for G in (1, 8):
        for weights in (None, w):
            for tr in (None, truth):
                m = f.ensemble_moments(weights, tr, groups=G)
                assert np.abs(m["spread"]).max() <= 1e-24, (G, np.abs(m["spread"]).max())
                np.testing.assert_allclose(m["mean_cov"], np.broadcast_to(P[0], (G, N, N)), rtol=1e-14, atol=0)
                if tr is None:
                    for g in range(G):
                        assert np.abs(o.boxminus(lay, m["center"][g], mean[0])).max() <= 1e-12
                else:
                    np.testing.assert_allclose(m["center"], np.broadcast_to(o.boxminus(lay, truth[0], mean[0]), (G, N)),
                                               rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", er.SHAPE_IDS)
def test_one_hot_weights(slk, name):
    """the centre is that filter's mean, mean_cov its P bit for bit on the lower triangle"""
    B = er.SHAPES[er.SHAPE_IDS.index(name)][3]
    for G in (1, 8):
        b = er.bank(name, G)
        lay, N, Bg = b["lay"], b["N"], B // G
        w = er.weights_of("onehot", B, G)
        hot = np.flatnonzero(w)
        f = make_filter(slk, b)
        m = f.ensemble_moments(w, None, groups=G, ess=True)
        il = np.tril_indices(N)
        for g in range(G):
            assert np.abs(o.boxminus(lay, m["center"][g], b["mean"][hot[g]])).max() <= 1e-12
            assert m["mean_cov"][g][il].tobytes() == b["P"][hot[g]][il].tobytes()
        assert (m["ess"] == 1.0).all()
        m6 = f.ensemble_moments(w, None, 3, 6, groups=G)
        for g in range(G):
            il6 = np.tril_indices(6)
            assert m6["mean_cov"][g][il6].tobytes() == b["P"][hot[g], 3:9, 3:9][il6].tobytes()


@pytest.mark.parametrize("mode", ["error", "mixture"])
def test_refused_groups_are_nan_and_alone(slk, mode):
    """a group of all-zero weights, one with a NaN, a negative and an infinite weight: only those groups are NaN"""
    G = 8
    b = er.bank("msckf_n60", G)
    B, Bg, lay = b["B"], b["B"] // G, b["lay"]
    truth = er.truth_of(b) if mode == "error" else None
    w = np.random.default_rng(5).uniform(0.5, 1.5, B)
    clean = w.copy()
    w[1 * Bg:2 * Bg] = 0.0
    w[3 * Bg + 17] = np.nan
    w[4 * Bg + 1] = -0.5
    w[6 * Bg + 5] = np.inf
    bad = [1, 3, 4, 6]
    good = [g for g in range(G) if g not in bad]
    f = make_filter(slk, b)
    f.clear_status()
    for t0, n in [(0, b["N"]), (0, 6)]:
        m = f.ensemble_moments(w, truth, t0, n, groups=G, ess=True)
        mc = f.ensemble_moments(clean, truth, t0, n, groups=G, ess=True)
        for k in m:
            assert np.isnan(m[k][bad]).all(), k
            assert m[k][good].tobytes() == mc[k][good].tobytes(), k
    assert (f.status() == 0).all()


# ------------------------------------------------------------------ 3. a lower-only covariance
def stepped(slk, kind, s, steps=2):
    if kind == "msckf":
        f = slk.Msckf(s["mean"], s["P"])
        for _ in range(steps):
            f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    else:
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
        for _ in range(steps):
            f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
    return f


def one_more(slk, kind, f, s):
    if kind == "msckf":
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    else:
        f.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"])
        f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"], gate=0)


@pytest.mark.parametrize("kind", ["msckf", "usckf"])
def test_after_fast_path_steps(slk, kind):
    """The exact-shape steps leave P lower-only.  The moments equal the twin on the (mu, P) a twin handle reports, and
    further steps are bit-identical to a handle that never made the call."""
    B, G = 64, 4
    b, s = er.step_inputs("msckf_n60" if kind == "msckf" else "usckf_n48", G, B)
    lay = b["lay"]
    f, other = stepped(slk, kind, s), stepped(slk, kind, s)
    mu, P = other.muState(), other._getP()                  # (completes the twin handle's P; f stays lower-only)
    w = np.random.default_rng(6).uniform(0.1, 1.0, B)
    truth = np.stack([o.boxplus(lay, mu[i], np.random.default_rng(i).normal(0, 0.05, s["N"])) for i in range(B)])
    for tr in (None, truth):
        for t0, n in [(0, s["N"]), (4, 5)]:
            got = f.ensemble_moments(w, tr, t0, n, groups=G, ess=True)
            twin = er.Twin(lay, mu, w, tr, G)
            assert twin.passes.max() < 20
            er.check_against_twin(lay, got, twin.moments(P, t0, n), tr is not None, f"{kind} lower-only")
    fresh = stepped(slk, kind, s)
    one_more(slk, kind, f, s)
    one_more(slk, kind, fresh, s)
    for x, y in zip(snapshot(f), snapshot(fresh)):
        assert x.tobytes() == y.tobytes()


def test_upper_triangle_is_never_read(slk):
    b = er.bank("msckf_n60", 8)
    N = b["N"]
    Pn = b["P"].copy()
    iu = np.triu_indices(N, 1)
    Pn[:, iu[0], iu[1]] = np.nan
    f, g = make_filter(slk, b), make_filter(slk, b, P=Pn)
    for t0, n in [(0, N), (4, 5)]:
        same_bits(f.ensemble_moments(None, None, t0, n, groups=8), g.ensemble_moments(None, None, t0, n, groups=8))


# ------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_handle_untouched(slk):
    B = 12
    s = sc.synthetic_msckf(B, 1, seed=0x4EF)
    f = slk.Msckf(s["mean"], s["P"])
    N, Nq = s["N"], s["Nq"]
    before = snapshot(f)
    ptrs = f.device_pointers()
    code = "slk_ensemble_moments failed with code -1"
    for t0, n in [(-1, 3), (0, 0), (0, -2), (N - 5, 6), (N, 1), (1, N)]:
        with pytest.raises(slk.SlkError, match=code):
            f.ensemble_moments(None, None, t0, n)
        with pytest.raises(slk.SlkError, match=code):
            f.ensemble_moments(None, s["mean"], t0, n)
    for G in (0, -1, 5, 7, 24):
        with pytest.raises(slk.SlkError, match=code):
            f.ensemble_moments(groups=G)
    lib, h = f._lib, f._h
    out = np.empty(N * N)
    assert lib.slk_ensemble_moments(h, 1, None, None, 0, N, None, None, None, None, slk.HOST) == slk.E_INVALID
    assert lib.slk_ensemble_moments(h, 1, None, None, 0, N, None, out.ctypes.data, None, None, 2) == slk.E_INVALID
    # everything NULL except ess is allowed, and so is any single output
    ess = np.empty(3)
    assert lib.slk_ensemble_moments(h, 3, None, None, 0, N, None, None, None, ess.ctypes.data, slk.HOST) == 0
    assert (ess == 4.0).all()
    assert lib.slk_ensemble_moments(h, 1, None, None, 0, N, None, out.ctypes.data, None, None, slk.HOST) == 0
    assert lib.slk_ensemble_moments(h, 1, None, None, 0, N, None, None, out.ctypes.data, None, slk.HOST) == 0
    np.testing.assert_allclose(out.reshape(N, N), s["P"].mean(axis=0), rtol=1e-12, atol=1e-17)
    cen = np.empty(Nq)
    assert lib.slk_ensemble_moments(h, 1, None, None, 0, N, cen.ctypes.data, None, None, None, slk.HOST) == 0
    for x, y in zip(before, snapshot(f)):
        assert x.tobytes() == y.tobytes()
    assert f.device_pointers() == ptrs


def test_full_batch_consistency_of_a_monte_carlo_run(slk):
    """error mode at N = 60, B = 4096: truth drawn from each filter's own Gaussian, so spread ~ mean_cov"""
    b = er.bank("msckf_n60", 1)
    truth = er.truth_of(b)
    f = make_filter(slk, b)
    m = f.ensemble_moments(None, truth)
    d = np.sqrt(np.diag(m["mean_cov"][0]))
    assert np.abs((m["spread"][0] - m["mean_cov"][0]) / np.outer(d, d)).max() < 0.15      # (B = 4096: 1 / sqrt(B) = 0.016)
    assert np.abs(m["center"][0] / d).max() < 0.1
