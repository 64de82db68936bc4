"""Multi-step trajectories (slk_step_n / step_n): T fused steps in one call against T single steps (bit-identical state,
status, outliers and per-step records on every launch route), shared inputs, interleaving with single steps, NEES
records against slk_nees, a failing filter, the device route, host-side rejection, and a 30-step run against the
oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc

pytestmark = pytest.mark.gpu

FEAT, POSE, VO = 2, 3, 1          # SLK_MM_FEATURE_PROJ, SLK_MM_POSE_POSITION, SLK_MM_VO_RELATIVE


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


class Case:
    """One filter shape with T steps of inputs: u [T, B, nu] and z [T, B, m] vary per step, params [B, np] per filter."""

    def __init__(self, kind, B, T, k=0, m=8, model=FEAT, nfk=3, nfkl=9, seed=0x7A11):
        rng = np.random.default_rng(seed)
        self.kind, self.B, self.T, self.m, self.model = kind, B, T, m, model
        if kind == "msckf":
            s = sc.synthetic_msckf(B, k, m=m if model == FEAT else 8, seed=seed)
            self.k, self.pm, self.gate = k, 2, (1 if model == FEAT else 0)
            if model == FEAT:
                self.params, z0 = s["feat"].reshape(B, -1), s["z"]
            else:
                self.params = np.zeros((B, 1))
                z0 = s["mean"][:, 0:3] + rng.normal(0, 0.05, (B, 3))
        else:
            s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=seed)
            self.nfk, self.nfkl, self.pm, self.gate = nfk, nfkl, 1, 0
            if model == FEAT:
                feat, z0 = sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(m // 2)), seed=seed + 1)
                self.params = feat.reshape(B, -1)
            else:
                self.params, z0 = None, s["z"]
        self.s = s
        self.Q, self.R = s["Q"], 0.01 * np.eye(m)
        nu = s["u"].shape[1]
        self.u = np.ascontiguousarray(s["u"][None] + np.concatenate(
            [rng.normal(0, 0.01, (T, B, 3)), np.zeros((T, B, nu - 3))], axis=2))
        if kind == "msckf":                                    # dquat stays a unit quaternion
            self.u[:, :, 3:7] = s["u"][None, :, 3:7]
        self.z = np.ascontiguousarray(z0[None] + rng.normal(0, 0.02, (T, B, m)))

    def filt(self, slk, P=None):
        P = self.s["P"] if P is None else P
        if self.kind == "msckf":
            return slk.Msckf(self.s["mean"], P)
        return slk.Usckf(mean=self.s["mean"], P=P, nfk=self.nfk, nfkl=self.nfkl)

    def single(self, f, t):
        f.step(self.pm, self.u[t], self.Q, self.z[t], self.model, self.params, self.R, gate=self.gate)

    def params_t(self):
        return None if self.params is None else np.broadcast_to(self.params, (self.T,) + self.params.shape)


def state(f):
    return f.muState(), f._getP(), f.status(), f.outliers()


def assert_nees(got, want, exact):
    """bit-identical where slk_step_n runs slk_nees's own kernel (ranges of n > 30); 1e-10 relative where it runs the
    one-wave register factorisation (n <= 30), NaN exactly where slk_nees has NaN"""
    if exact:
        np.testing.assert_array_equal(got, want)
        return
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok])), float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])))


def assert_same_state(fa, fb):
    for x, y in zip(state(fa), state(fb)):
        np.testing.assert_array_equal(x, y)


ROUTES = [
    ("msckf-N12-pose-closed-form", dict(kind="msckf", B=16, k=0, m=3, model=POSE)),
    ("msckf-N12-m4", dict(kind="msckf", B=16, k=0, m=4)),
    ("msckf-N18-m2", dict(kind="msckf", B=16, k=1, m=2)),
    ("msckf-N18-m6", dict(kind="msckf", B=16, k=1, m=6)),
    ("msckf-N30-m8", dict(kind="msckf", B=16, k=3, m=8)),
    ("msckf-N12-B8192", dict(kind="msckf", B=8192, k=0, m=4)),
    ("msckf-N60-fast-lower-only", dict(kind="msckf", B=16, k=8, m=8)),
    ("msckf-N60-general", dict(kind="msckf", B=16, k=8, m=6)),
    ("msckf-N84-large", dict(kind="msckf", B=16, k=12, m=8)),
    ("usckf-N48-split-lower-only", dict(kind="usckf", B=16, nfk=3, nfkl=9, m=3, model=VO)),
    ("usckf-N48-wide-m40", dict(kind="usckf", B=16, nfk=3, nfkl=9, m=40, model=FEAT)),
]


# ------------------------------------------------------------------ 1. bit-identical to single steps, every route
@pytest.mark.parametrize("spec", [r[1] for r in ROUTES], ids=[r[0] for r in ROUTES])
def test_step_n_equals_single_steps(slk, spec):
    T = 7
    c = Case(T=T, **spec)
    fs, fn = c.filt(slk), c.filt(slk)
    means, outs = [], []
    for t in range(T):
        c.single(fs, t)
        means.append(fs.muState())
        outs.append(fs.outliers())
    rec = fn.step_n(c.pm, c.u, c.Q, c.z, c.model, c.params_t(), c.R, gate=c.gate, record_mean=True, record_outliers=True)
    assert_same_state(fs, fn)
    for t in range(T):
        np.testing.assert_array_equal(rec["mean"][t], means[t])
        np.testing.assert_array_equal(rec["outliers"][t], outs[t])
    st = fs.status()
    assert (st & slk.ST_LLT_FAIL == 0).all()


# ------------------------------------------------------------------ 2. shared inputs (every per-step stride 0)
@pytest.mark.parametrize("spec", [dict(kind="msckf", B=16, k=1, m=6), dict(kind="usckf", B=8, nfk=3, nfkl=9, m=3, model=VO)],
                         ids=["msckf-N18", "usckf-N48"])
def test_step_n_shared_inputs(slk, spec):
    T = 5
    c = Case(T=T, **spec)
    fs, fn = c.filt(slk), c.filt(slk)
    for _ in range(T):
        fs.step(c.pm, c.u[0], c.Q, c.z[0], c.model, c.params, c.R, gate=c.gate)
    u = np.broadcast_to(c.u[0], c.u.shape)
    z = np.broadcast_to(c.z[0], c.z.shape)
    rec = fn.step_n(c.pm, u, c.Q, z, c.model, c.params_t(), c.R, gate=c.gate, record_mean=True)
    assert_same_state(fs, fn)
    np.testing.assert_array_equal(rec["mean"][-1], fs.muState())


# ------------------------------------------------------------------ 3. interleaving with single steps
@pytest.mark.parametrize("spec", [dict(kind="msckf", B=16, k=8, m=8), dict(kind="msckf", B=16, k=0, m=3, model=POSE)],
                         ids=["N60-lower-only", "N12"])
def test_step_n_interleaves_with_single_steps(slk, spec):
    c = Case(T=5, **spec)
    fs, fn = c.filt(slk), c.filt(slk)
    for t in range(5):
        c.single(fs, t)
    c.single(fn, 0)
    p = None if c.params is None else np.broadcast_to(c.params, (3,) + c.params.shape)
    fn.step_n(c.pm, c.u[1:4], c.Q, c.z[1:4], c.model, p, c.R, gate=c.gate)
    c.single(fn, 4)
    assert_same_state(fs, fn)


# ------------------------------------------------------------------ 4. NEES records against slk_nees
@pytest.mark.parametrize("spec", [dict(kind="msckf", B=16, k=0, m=3, model=POSE), dict(kind="msckf", B=16, k=1, m=6),
                                  dict(kind="msckf", B=16, k=3, m=8), dict(kind="msckf", B=16, k=8, m=8),
                                  dict(kind="usckf", B=8, nfk=3, nfkl=9, m=3, model=VO)],
                         ids=["msckf-N12", "msckf-N18", "msckf-N30", "msckf-N60", "usckf-N48"])
@pytest.mark.parametrize("rng_", [None, (4, 7)], ids=["full", "t0-4-n7"])
def test_step_n_nees_records(slk, spec, rng_):
    T = 6
    c = Case(T=T, **spec)
    r = np.random.default_rng(31)
    truth = np.repeat(c.s["mean"][None], T, axis=0)
    truth[:, :, 0:3] += r.normal(0, 0.05, (T, c.B, 3))
    fs, fn = c.filt(slk), c.filt(slk)
    t0, n = (0, fs.N) if rng_ is None else rng_
    want = []
    for t in range(T):
        c.single(fs, t)
        want.append(fs.nees(truth[t], t0, n))
    rec = fn.step_n(c.pm, c.u, c.Q, c.z, c.model, c.params_t(), c.R, gate=c.gate, truth=truth, nees_range=rng_)
    assert_nees(rec["nees"], np.array(want), exact=n > 30)
    assert np.isfinite(rec["nees"]).all()
    assert_same_state(fs, fn)


# ------------------------------------------------------------------ 5. a failing filter
def test_step_n_failing_filter(slk):
    T = 4
    c = Case(T=T, kind="msckf", B=16, k=1, m=6)
    P = c.s["P"].copy()
    P[5] = -P[5]                                             # indefinite: every factorisation of filter 5 fails
    truth = np.repeat(c.s["mean"][None], T, axis=0)
    fs, fn = c.filt(slk, P), c.filt(slk, P)
    want = []
    for t in range(T):
        c.single(fs, t)
        want.append(fs.nees(truth[t]))
    rec = fn.step_n(c.pm, c.u, c.Q, c.z, c.model, c.params_t(), c.R, gate=c.gate, truth=truth)
    assert_same_state(fs, fn)
    st = fn.status()
    assert st[5] & slk.ST_LLT_FAIL
    assert (np.delete(st, 5) & slk.ST_LLT_FAIL == 0).all()
    np.testing.assert_array_equal(fn.muState()[5], c.s["mean"][5])
    assert np.isnan(rec["nees"][:, 5]).all()
    assert np.isfinite(np.delete(rec["nees"], 5, axis=1)).all()
    assert_nees(rec["nees"], np.array(want), exact=False)


# ------------------------------------------------------------------ 6. device route == host route
@pytest.mark.parametrize("spec", [dict(kind="msckf", B=16, k=0, m=4), dict(kind="msckf", B=16, k=8, m=8)], ids=["N12", "N60"])
def test_step_n_device_route(slk, spec):
    import torch
    T = 5
    c = Case(T=T, **spec)
    truth = np.repeat(c.s["mean"][None], T, axis=0)
    fh, fd = c.filt(slk), c.filt(slk)
    rh = fh.step_n(c.pm, c.u, c.Q, c.z, c.model, c.params_t(), c.R, gate=c.gate, truth=truth, record_mean=True,
                   record_outliers=True)
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    pd = d(c.params).unsqueeze(0).expand(T, *c.params.shape)            # one block for every step (stride 0)
    rd = fd.step_n(c.pm, d(c.u), d(c.Q), d(c.z), c.model, pd, d(c.R), gate=c.gate, truth=d(truth), record_mean=True,
                   record_outliers=True)
    assert all(v.is_cuda for v in rd.values())
    np.testing.assert_array_equal(rd["mean"].cpu().numpy(), rh["mean"])
    np.testing.assert_array_equal(rd["nees"].cpu().numpy(), rh["nees"])
    assert rd["outliers"].dtype == torch.uint32
    np.testing.assert_array_equal(rd["outliers"].cpu().numpy(), rh["outliers"])
    assert_same_state(fh, fd)


# ------------------------------------------------------------------ 7. host-side rejection leaves the filter untouched
def test_step_n_rejects_bad_calls(slk):
    lib = slk.load_library()
    T, B, k, m = 3, 8, 1, 6
    c = Case(T=T, kind="msckf", B=B, k=k, m=m)
    f = c.filt(slk)
    c.single(f, 0)
    before = state(f)
    Q = np.ascontiguousarray(c.Q.T)
    R = np.ascontiguousarray(c.R.T)
    z33 = np.zeros((T, B, 34))
    R33 = np.eye(34) * 0.01
    truth = np.repeat(c.s["mean"][None], T, axis=0)
    nees = np.empty((T, B))

    def traj(**kw):
        t = slk.Traj()
        t.T, t.pmodel, t.u, t.u_stride, t.u_tstride = T, c.pm, c.u.ctypes.data, 13, B * 13
        t.Q, t.q_stride, t.q_tstride = Q.ctypes.data, 0, 0
        t.mmodel, t.params, t.p_stride, t.p_tstride = FEAT, c.params.ctypes.data, c.params.shape[1], 0
        t.z, t.m, t.z_tstride = c.z.ctypes.data, m, B * m
        t.R, t.r_stride, t.r_tstride = R.ctypes.data, 0, 0
        t.gate = 1
        for key, v in kw.items():
            setattr(t, key, v)
        return t

    bad = {
        "T0": traj(T=0),
        "null-z": traj(z=None),
        "nees-without-truth": traj(nees_hist=nees.ctypes.data),
        "short-tstride": traj(z_tstride=B * m - 1),
        "negative-tstride": traj(u_tstride=-13 * B),
        "msckf-m33": traj(z=z33.ctypes.data, m=33, z_tstride=B * 33, R=R33.ctypes.data),
        "msckf-m34": traj(z=z33.ctypes.data, m=34, z_tstride=B * 34, R=R33.ctypes.data),
        "external-model": traj(mmodel=slk.MODEL_EXTERNAL),
        "unknown-where": None,
        "bad-nees-range": traj(truth=truth.ctypes.data, truth_tstride=B * f.Nq, nees_t0=10, nees_n=9, nees_hist=nees.ctypes.data),
    }
    for name, t in bad.items():
        where = slk.HOST
        if t is None:
            t, where = traj(), 2
        assert lib.slk_step_n(f._h, C.byref(t), where) == slk.E_INVALID, name
        for x, y in zip(before, state(f)):
            np.testing.assert_array_equal(x, y, err_msg=name)
    assert lib.slk_step_n(f._h, C.byref(traj()), slk.HOST) == 0      # the unmodified call is accepted


# ------------------------------------------------------------------ 7b. mis-shaped inputs are refused by the wrapper
def test_step_n_wrapper_refuses_misshaped_inputs(slk):
    T, B = 3, 8
    c = Case(T=T, kind="msckf", B=B, k=1, m=6)
    f = c.filt(slk)
    before = state(f)
    p = c.params_t()
    truth = np.repeat(c.s["mean"][None], T, axis=0)
    bad = {
        "z-broadcast-short-B": dict(z=np.broadcast_to(c.z[0, :B - 1], (T, B - 1, 6))),
        "z-wider-B": dict(z=np.zeros((T, B + 1, 6))),
        "z-shared-row": dict(z=c.z[:, 0]),
        "u-broadcast-short-B": dict(u=np.broadcast_to(c.u[0, :B - 1], (T, B - 1, 13))),
        "u-narrow": dict(u=c.u[:, :, :12]),
        "params-broadcast-short-B": dict(params=np.broadcast_to(c.params[:B - 1], (T, B - 1, c.params.shape[1]))),
        "params-narrow": dict(params=p[:, :, :-1]),
        "truth-short-Nq": dict(truth=np.broadcast_to(truth[0, :, :-1], (T, B, f.Nq - 1))),
        "truth-short-B": dict(truth=truth[:, :B - 1]),
        "T-mismatch": dict(u=c.u[:T - 1]),
    }
    for name, kw in bad.items():
        args = dict(u=c.u, z=c.z, params=p, truth=None)
        args.update(kw)
        with pytest.raises(slk.SlkError):
            f.step_n(c.pm, args["u"], c.Q, args["z"], c.model, args["params"], c.R, gate=c.gate, truth=args["truth"])
        for x, y in zip(before, state(f)):
            np.testing.assert_array_equal(x, y, err_msg=name)


# ------------------------------------------------------------------ 8. a 30-step N = 12 trajectory against the oracle
def test_step_n_trajectory_stays_on_the_oracle(slk):
    B, k, m, T = 12, 0, 4, 30
    s = sc.synthetic_msckf(B, k, m=m, seed=2025)
    lay = o.layout(o.MULTI, k)
    N = s["N"]
    rng = np.random.default_rng(6)
    U = np.repeat(s["u"][None], T, axis=0)
    U[:, :, 0:3] += rng.normal(0, 0.02, (T, B, 3))
    Z = s["z"][None] + rng.normal(0, 0.02, (T, B, m))
    f = slk.Msckf(s["mean"], s["P"])
    feat = s["feat"].reshape(B, -1)
    rec = f.step_n(slk.PM_DELTA_POSE, U, s["Q"], Z, slk.MM_FEATURE_PROJ, np.broadcast_to(feat, (T,) + feat.shape), s["R"],
                   record_mean=True, record_outliers=True)
    assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
    mean, P = s["mean"].copy(), s["P"].copy()
    for t in range(T):
        st, out = o.msckf_step_batch(k, m, 1, mean, P, np.ascontiguousarray(U[t]), s["feat"], np.ascontiguousarray(Z[t]),
                                     s["Q"], s["R"])
        assert st == 0
        np.testing.assert_array_equal(rec["outliers"][t], out)
        for b in range(B):
            assert float(np.abs(o.boxminus(lay, rec["mean"][t, b], mean[b])).max()) <= 1e-8, (t, b)
    Pg = f.getPk()
    for b in range(B):
        assert rel(Pg[b], P[b].reshape(N, N).T) <= 1e-8, b
