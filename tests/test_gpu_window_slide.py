"""Sliding-window Msckf trajectories: slk_msckf_slide / Msckf.slide (drop a clone and clone the current pose in one
launch) against drop_clone + clone_pose, bit for bit, on every step kernel's window; every kind of follow-up call on a
lower-only covariance right after a slide; slk_step_n_slide / step_n(slide=...) against the loop of single steps and
window operations (state and records, host and device routes); a sliding 20-step trajectory against the oracle;
refusals; and the zero-copy pointer after a slide."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc

pytestmark = pytest.mark.gpu

FEAT = 2                           # SLK_MM_FEATURE_PROJ


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def slide_maps(k, d):
    """(tangent, storage) source index of every new index after dropping clone d and cloning the pose"""
    N, Nq = 12 + 6 * k, 13 + 7 * k
    tan = [t - (N - 6) if t >= N - 6 else (t if t < 12 + 6 * d else t + 6) for t in range(N)]
    sto = [e - (Nq - 7) if e >= Nq - 7 else (e if e < 13 + 7 * d else e + 7) for e in range(Nq)]
    return np.array(tan), np.array(sto)


def state(f):
    return f.muState(), f._getP(), f.status(), f.outliers()


def assert_same(fa, fb):
    for x, y in zip(state(fa), state(fb)):
        np.testing.assert_array_equal(x, y)


class Twins:
    """Msckf handles on the same inputs: `steps` fused m-row feature steps each (k = 4 .. 8 with m = 8: the exact-shape
    fast path, which leaves P lower-only)"""

    def __init__(self, slk, B, k, m=8, seed=0x511DE):
        self.slk, self.B, self.k, self.m = slk, B, k, m
        self.s = sc.synthetic_msckf(B, k, m=m, seed=seed)
        rng = np.random.default_rng(seed + 1)
        self.u = [self.s["u"] + np.concatenate([rng.normal(0, 0.01, (B, 3)), np.zeros((B, 10))], axis=1) for _ in range(4)]
        for u in self.u:
            u[:, 3:7] = self.s["u"][:, 3:7]
        self.z = [self.s["z"] + rng.normal(0, 0.02, (B, m)) for _ in range(4)]
        self.params = self.s["feat"].reshape(B, -1)

    def step(self, f, t):
        f.step(self.slk.PM_DELTA_POSE, self.u[t], self.s["Q"], self.z[t], FEAT, self.params, self.s["R"])

    def make(self, steps=2):
        f = self.slk.Msckf(self.s["mean"], self.s["P"])
        for t in range(steps):
            self.step(f, t)
        return f


def slide_cases():
    out = []
    for k in (1, 4, 8, 9, 31, 33):
        for d in sorted({0, k // 2, k - 1}):
            out.append(pytest.param(3, k, d, id=f"B3-k{k}-d{d}"))
    out += [pytest.param(4096, 8, d, id=f"B4096-k8-d{d}") for d in (0, 7)]
    return out


# ------------------------------------------------------------------ 1. slide == drop_clone + clone_pose, bit for bit
@pytest.mark.parametrize("B,k,d", slide_cases())
def test_slide_equals_drop_then_clone(slk, B, k, d):
    tw = Twins(slk, B, k)
    fa, fb, fc = tw.make(), tw.make(), tw.make()
    fa.slide(d)
    fb.drop_clone(d)
    fb.clone_pose()
    assert fa.N == fb.N == 12 + 6 * k and fa.Nq == fb.Nq
    np.testing.assert_array_equal(fa.muState(), fb.muState())
    np.testing.assert_array_equal(fa.getPk(), fb.getPk())
    # and the permutation itself, on the state the slide started from
    tan, sto = slide_maps(k, d)
    Mc, Pc = fc.muState(), fc.getPk()
    np.testing.assert_array_equal(fa.muState(), Mc[:, sto])
    np.testing.assert_array_equal(fa.getPk(), Pc[:, tan][:, :, tan])


# ------------------------------------------------------------------ 2. every kind of call right after a slide
FOLLOW_UPS = ["fast-step", "m4-update", "ekf-update", "nees", "sample-states", "check-sigma-points"]


@pytest.mark.parametrize("what", FOLLOW_UPS)
@pytest.mark.parametrize("d", [0, 5])
def test_calls_after_a_slide(slk, what, d):
    B, k = 3, 8
    tw = Twins(slk, B, k)
    fa, fb = tw.make(), tw.make()
    fa.slide(d)                         # lower-only in, lower-only out: no read-out before the follow-up call
    fb.drop_clone(d)
    fb.clone_pose()
    N = fa.N
    rng = np.random.default_rng(77)
    if what == "fast-step":
        for f in (fa, fb):
            tw.step(f, 2)
    elif what == "m4-update":
        p4, z4 = tw.params[:, :8], tw.z[2][:, :4]
        for f in (fa, fb):
            f.update(z4, FEAT, p4, 0.01 * np.eye(4))
    elif what == "ekf-update":
        e = sc.synthetic_ekf(B, k, N + 8, seed=99, outliers=False)
        for f in (fa, fb):
            f.update_ekf(e["z"], e["zmean"], e["H"], e["R"], gate=False)
    elif what == "nees":
        truth = fb.muState()
        truth[:, 0:3] += rng.normal(0, 0.05, (B, 3))
        np.testing.assert_array_equal(fa.nees(truth), fb.nees(truth))
        np.testing.assert_array_equal(fa.nees(truth, N - 6, 6), fb.nees(truth, N - 6, 6))
    elif what == "sample-states":
        noise = rng.normal(0, 1, (B, 4, N))
        np.testing.assert_array_equal(fa.sample_states(noise), fb.sample_states(noise))
    else:
        # right after a slide the newest clone equals the pose, so P is singular and its factor undefined: one
        # predict (process noise on the pose) first, still with no read-out of the slid state
        for f in (fa, fb):
            f.predict(slk.PM_DELTA_POSE, tw.u[2], tw.s["Q"])
        ca, cb = fa.checkSigmaPoints(), fb.checkSigmaPoints()
        np.testing.assert_array_equal(ca[0], cb[0])
        np.testing.assert_array_equal(ca[1], cb[1])
        assert (ca[0] <= 1e-6).all()
    assert_same(fa, fb)


# ------------------------------------------------------------------ 3. step_n(slide=...) == the loop
class Traj:
    def __init__(self, slk, B, k, m, T, seed=0x7A1D):
        self.slk, self.B, self.k, self.m, self.T = slk, B, k, m, T
        s = sc.synthetic_msckf(B, k, m=m, seed=seed)
        rng = np.random.default_rng(seed)
        self.s = s
        self.u = np.repeat(s["u"][None], T, axis=0)
        self.u[:, :, 0:3] += rng.normal(0, 0.01, (T, B, 3))
        self.z = np.ascontiguousarray(s["z"][None] + rng.normal(0, 0.02, (T, B, m)))
        self.params = s["feat"].reshape(B, -1)
        self.truth = np.repeat(s["mean"][None], T, axis=0)
        self.truth[:, :, 0:3] += rng.normal(0, 0.05, (T, B, 3))

    def filt(self):
        return self.slk.Msckf(self.s["mean"], self.s["P"])

    def loop(self, f, sched, t0, n):
        means, outs, nees = [], [], []
        for t in range(self.T):
            f.step(self.slk.PM_DELTA_POSE, self.u[t], self.s["Q"], self.z[t], FEAT, self.params, self.s["R"])
            if sched[t] >= 0:
                f.drop_clone(int(sched[t]))
                f.clone_pose()
            means.append(f.muState())
            outs.append(f.outliers())
            nees.append(f.nees(self.truth[t], t0, n))
        return np.array(means), np.array(outs), np.array(nees)

    def step_n(self, f, sched, t0, n, device=False):
        p = np.broadcast_to(self.params, (self.T,) + self.params.shape)
        u, Q, z, R, truth = self.u, self.s["Q"], self.z, self.s["R"], self.truth
        if device:
            import torch
            dev = torch.device("cuda:0")
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
            u, Q, z, R, truth = d(u), d(Q), d(z), d(R), d(truth)
            p = d(self.params).unsqueeze(0).expand(self.T, *self.params.shape)
        rec = f.step_n(self.slk.PM_DELTA_POSE, u, Q, z, FEAT, p, R, truth=truth, nees_range=(t0, n), record_mean=True,
                       record_outliers=True, slide=sched)
        if device:
            rec = {key: v.cpu().numpy() for key, v in rec.items()}
        return rec


def assert_nees(got, want, exact):
    """bit-identical where slk_step_n runs slk_nees's own kernel (n > 30); 1e-10 relative where it runs its one-wave
    record kernel (n <= 30), NaN exactly where slk_nees has NaN (the rule of slk_step_n's NEES records)"""
    if exact:
        np.testing.assert_array_equal(got, want)
        return
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok]))


SPECS = [pytest.param(8, 8, id="k8-m8-fast"), pytest.param(4, 4, id="k4-m4"), pytest.param(1, 2, id="k1-m2")]
SCHEDS = ["none", "every-0", "mixed"]


def schedule(kind, T, k):
    if kind == "none":
        return np.full(T, -1)
    if kind == "every-0":
        return np.zeros(T, dtype=int)
    return np.array([0, -1, k - 1, -1, k // 2, 0][:T])


@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("k,m", SPECS)
@pytest.mark.parametrize("rng_", ["state", "clone", "older"])
def test_step_n_slide_equals_the_loop(slk, k, m, sched, rng_):
    T, B = 6, 16
    tr = Traj(slk, B, k, m, T)
    N = 12 + 6 * k
    # (the whole state is singular after a slide: the newest clone equals the pose; "older" leaves it out)
    t0, n = {"state": (0, 12), "clone": (12, 6), "older": (0, N - 6)}[rng_]
    sch = schedule(sched, T, k)
    fl, fh = tr.filt(), tr.filt()
    means, outs, nees = tr.loop(fl, sch, t0, n)
    rec = tr.step_n(fh, sch, t0, n)
    assert_same(fl, fh)
    np.testing.assert_array_equal(rec["mean"], means)
    np.testing.assert_array_equal(rec["outliers"], outs)
    assert_nees(rec["nees"], nees, exact=n > 30)
    assert np.isfinite(rec["nees"]).all()
    assert (fh.status() & slk.ST_LLT_FAIL == 0).all()
    # the device route (torch tensors) == the host route
    fd = tr.filt()
    recd = tr.step_n(fd, [int(x) for x in sch], t0, n, device=True)
    for key in rec:
        np.testing.assert_array_equal(recd[key], rec[key])
    assert_same(fd, fh)


def test_step_n_without_a_schedule_is_step_n(slk):
    tr = Traj(slk, 16, 8, 8, 5)
    fa, fb = tr.filt(), tr.filt()
    ra = tr.step_n(fa, None, 0, 12)
    rb = tr.step_n(fb, [-1] * 5, 0, 12)
    assert_same(fa, fb)
    for key in ra:
        np.testing.assert_array_equal(ra[key], rb[key])


# ------------------------------------------------------------------ 4. a sliding trajectory against the oracle
def test_sliding_trajectory_stays_on_the_oracle(slk):
    B, k, m, T = 12, 4, 8, 20
    s = sc.synthetic_msckf(B, k, m=m, seed=2026)
    lay = o.layout(o.MULTI, k)
    N, Nq = s["N"], s["Nq"]
    rng = np.random.default_rng(8)
    U = np.repeat(s["u"][None], T, axis=0)
    U[:, :, 0:3] += rng.normal(0, 0.02, (T, B, 3))
    tan, sto = slide_maps(k, 0)
    # per-step features: landmark j stays with the clone that saw it; it moves one slot down at every slide, and the
    # newest clone takes over a landmark whose clone has left the window.  z = the landmark seen from that slot of the
    # oracle's own state before the step, plus noise.
    lm = s["feat"][:, :, 0:3]
    slot0 = s["feat"][0, :, 3].astype(int)
    feats, Zs, want_mean, want_out = [], [], [], []
    mean, P = s["mean"].copy(), s["P"].copy()
    for t in range(T):
        slot = (slot0 - 1 - t) % k + 1
        feat = s["feat"].copy()
        feat[:, :, 3] = slot
        z = np.zeros((B, m))
        for j in range(m // 2):
            so = 13 + 7 * (slot[j] - 1)
            pos, q = mean[:, so:so + 3], mean[:, so + 3:so + 7]
            qc = np.concatenate([-q[:, :3], q[:, 3:]], axis=1)
            loc = sc.quat_rotate(qc, lm[:, j] - pos)
            z[:, 2 * j:2 * j + 2] = loc[:, 0:2] / loc[:, 2:3] + rng.normal(0, 0.02, (B, 2))
        feats.append(feat)
        Zs.append(z)
        st, out = o.msckf_step_batch(k, m, 1, mean, P, np.ascontiguousarray(U[t]), feat, z, s["Q"], s["R"])
        assert st == 0
        mean = np.ascontiguousarray(mean[:, sto])                                 # the slide, in numpy
        P = np.ascontiguousarray(P.reshape(B, N, N)[:, tan][:, :, tan].reshape(B, N * N))
        want_mean.append(mean.copy())
        want_out.append(out)
    f = slk.Msckf(s["mean"], s["P"])
    F = np.array([x.reshape(B, -1) for x in feats])
    rec = f.step_n(slk.PM_DELTA_POSE, U, s["Q"], np.array(Zs), FEAT, F, s["R"], record_mean=True, record_outliers=True,
                   slide=0)
    assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
    assert rec["outliers"].sum() <= rec["outliers"].size * (m // 2) // 2          # most features are used
    for t in range(T):
        np.testing.assert_array_equal(rec["outliers"][t], want_out[t])
        for b in range(B):
            assert float(np.abs(o.boxminus(lay, rec["mean"][t, b], want_mean[t][b])).max()) <= 1e-8, (t, b)
    Mg, Pg = f.muState(), f.getPk()
    np.testing.assert_array_equal(rec["mean"][-1], Mg)
    for b in range(B):
        Pb = P[b].reshape(N, N).T
        assert float(np.abs(Pg[b] - Pb).max() / np.abs(Pb).max()) <= 1e-8, b


# ------------------------------------------------------------------ 5. refusals leave the filter untouched
def test_refusals_leave_the_filter_untouched(slk):
    lib = slk.load_library()
    # Usckf: no window to slide, directly or in a trajectory
    su = sc.synthetic_usckf(4, nfk=3, nfkl=9, seed=3)
    fu = slk.Usckf(mean=su["mean"], P=su["P"], nfk=3, nfkl=9)
    before = state(fu)
    assert lib.slk_msckf_slide(fu._h, 0) == slk.E_INVALID
    T = 3
    u = np.broadcast_to(su["u"], (T,) + su["u"].shape)
    z = np.broadcast_to(su["z"], (T,) + su["z"].shape)
    with pytest.raises(slk.SlkError, match="slk_step_n_slide"):
        fu.step_n(slk.PM_CONST_VELOCITY, u, su["Q"], z, slk.MM_VO_RELATIVE, None, 0.01 * np.eye(z.shape[-1]), slide=-1)
    for x, y in zip(before, state(fu)):
        np.testing.assert_array_equal(x, y)
    # k = 0
    f0 = Twins(slk, 3, 0, m=4).make(1)
    before = state(f0)
    assert lib.slk_msckf_slide(f0._h, 0) == slk.E_INVALID
    with pytest.raises(slk.SlkError):
        f0.slide(0)
    for x, y in zip(before, state(f0)):
        np.testing.assert_array_equal(x, y)
    # indices outside 0 .. k - 1, on a lower-only covariance
    tw = Twins(slk, 3, 8)
    f, ref = tw.make(), tw.make()
    for idx in (-2, -1, 8, 9):
        assert lib.slk_msckf_slide(f._h, idx) == slk.E_INVALID, idx
    assert lib.slk_msckf_slide(None, 0) == slk.E_INVALID
    assert_same(f, ref)
    # a bad schedule entry at t = T - 1: nothing of steps 0 .. T - 2 has run
    tr = Traj(slk, 8, 4, 4, 4)
    f = tr.filt()
    before = state(f)
    for bad in ([0, 0, 0, 4], [0, -1, 1, -2], [3, 3, 3, 99]):
        with pytest.raises(slk.SlkError):
            tr.step_n(f, bad, 0, 12)
        for x, y in zip(before, state(f)):
            np.testing.assert_array_equal(x, y, err_msg=str(bad))
    # a wrong-length or non-integer schedule is refused by the wrapper before the call
    for bad in ([0] * 3, [0] * 5, [[0] * 4], np.zeros(4)):
        with pytest.raises(slk.SlkError, match="slide must be"):
            tr.step_n(f, bad, 0, 12)
    for x, y in zip(before, state(f)):
        np.testing.assert_array_equal(x, y)
    tr.step_n(f, [0, 0, 0, 3], 0, 12)                      # the well-formed call is accepted


# ------------------------------------------------------------------ 6. zero-copy after a slide
def test_device_pointers_after_a_slide(slk):
    import torch
    assert torch.cuda.is_available()
    tw = Twins(slk, 6, 8)
    f = tw.make()
    mean0, cov0 = f.device_pointers()
    f2 = tw.make()
    f.slide(3)
    f2.slide(3)
    mean1, cov1 = f.device_pointers()                       # completes the strict upper triangle on the handle's stream
    assert (mean1, cov1) != (mean0, cov0)                   # the state moved to the second buffer pair
    f.sync()
    B, N, Nq = f.B, f.N, f.Nq
    host, hmean = np.empty((B, N, N)), np.empty((B, Nq))
    rt = C.CDLL("libamdhip64.so")
    assert rt.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(cov1), C.c_size_t(host.nbytes), 2) == 0
    assert rt.hipMemcpy(C.c_void_p(hmean.ctypes.data), C.c_void_p(mean1), C.c_size_t(hmean.nbytes), 2) == 0
    P = f2.getPk()
    np.testing.assert_array_equal(np.transpose(host, (0, 2, 1)), P)
    np.testing.assert_array_equal(host, np.transpose(host, (0, 2, 1)))
    np.testing.assert_array_equal(hmean, f2.muState())
