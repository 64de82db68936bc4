"""Msckf EKF update from a registered measurement model (slk_ekf_linearize, slk_update_ekf_model, slk_step_ekf,
slk_step_n_ekf): the device linearisation against an analytic numpy Jacobian (ekf_model_ref.py, itself checked against
central differences of the oracle's model and boxplus by tests/test_ekf_model_host.py), bit-exact composition with
slk_update_ekf on both of its kernels, the update against the CPU oracle run one filter at a time, steps and trajectories
against loops of single calls, and every refusal.  Run with `pytest -m gpu` on an MI355X (`-s` prints the errors seen)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as o
import ekf_model_ref as ref
import scenarios as sc

pytestmark = pytest.mark.gpu

TOL = 1e-9                                    # the tolerance tests/test_gpu_ekf.py uses for this update
FEAT, POSE, VO, EXT = 2, 3, 1, 0
IDS = [f"k{k}-m{m}" for k, m in ref.SHAPES]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def on_device(f, call, *arrays):
    """call(*device tensors of the arrays), then wait for the handle's stream: the library reads device arguments
    asynchronously, so they must outlive the work (torch would hand their memory to the next tensor otherwise)."""
    t = [dev(a) for a in arrays]
    call(*t)
    f.sync()


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def state(f):
    return f.muState(), f.getPk(), f.status(), f.outliers()


def assert_same_state(fa, fb):
    for x, y in zip(state(fa), state(fb)):
        np.testing.assert_array_equal(x, y)


def params2(s):
    return s["feat"].reshape(s["B"], -1)


# ------------------------------------------------------------------ 1. the Jacobian
def check_linearisation(s, zm, H):
    """(b) zmean / H against numpy to 1e-12 * max(1, max|H|) per filter; (c) exact +0.0 outside the six columns of each
    row's pose, columns 6 .. 11 all zero, nothing left unwritten."""
    k, B, m, N = s["k"], s["B"], s["m"], s["N"]
    zr, Hr = ref.linearize_np(s["mean"], s["feat"], k)
    assert zm.shape == (B, m) and H.shape == (B, m, N)
    assert not np.isnan(zm).any() and not np.isnan(H).any(), "a store is missing"
    worst = 0.0
    for b in range(B):
        tol = 1e-12 * max(1.0, np.abs(Hr[b]).max())
        e = max(np.abs(H[b] - Hr[b]).max(), np.abs(zm[b] - zr[b]).max())
        assert e <= tol, (b, e, tol)
        worst = max(worst, e)
    c = s["feat"][..., 3].astype(int)
    tp = np.where(c == 0, 0, 12 + 6 * (c - 1))                                   # [B, nf]
    inside = np.zeros((B, m, N), dtype=bool)
    cols = np.arange(N)[None, None, :]
    for r in range(2):
        inside[:, r::2, :] = (cols >= tp[:, :, None]) & (cols < tp[:, :, None] + 6)
    bits = np.ascontiguousarray(H).view(np.uint64)
    assert (bits[~inside] == 0).all(), "an entry outside the pose's six columns is not +0.0"
    assert (bits[:, :, 6:12] == 0).all()
    return worst


@pytest.mark.parametrize("shared", [False, True], ids=["per_filter", "shared"])
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("k,m", ref.SHAPES, ids=IDS)
def test_jacobian(slk, k, m, route, shared):
    s = ref.scenario(k, m)
    if shared:                                                # the features of filter 0 for every filter
        s["feat"] = np.ascontiguousarray(np.broadcast_to(s["feat"][0], s["feat"].shape))
    f = slk.Msckf(s["mean"], s["P"])
    before = state(f)
    p = s["feat"][0].ravel() if shared else params2(s)
    if route == "device":
        zm, H = f.ekf_linearize(FEAT, dev(p), m)
        zm.fill_(float("nan"))                                # a second call into NaN-filled buffers: every entry is stored
        H.fill_(float("nan"))
        import torch
        torch.cuda.synchronize()
        lib = slk.load_library()
        pd = dev(p)
        assert lib.slk_ekf_linearize(f._h, FEAT, pd.data_ptr(), 0 if shared else int(pd.stride(0)), m, zm.data_ptr(),
                                     H.transpose(1, 2).data_ptr(), slk.DEVICE) == 0
        f.sync()
        zm, H = zm.cpu().numpy(), H.cpu().numpy()
    else:
        zm, H = f.ekf_linearize(FEAT, p, m)
    print(f"\nlinearisation k={k} m={m} {route}: worst abs error {check_linearisation(s, zm, H):.2e}")
    for x, y in zip(before, state(f)):                        # the filter is not modified
        np.testing.assert_array_equal(x, y)


def test_jacobian_full_batch(slk):
    s = ref.scenario(8, 128, B=1024)
    f = slk.Msckf(s["mean"], s["P"])
    zm, H = f.ekf_linearize(FEAT, dev(params2(s)), 128)
    print(f"\nlinearisation B=1024: worst abs error {check_linearisation(s, zm.cpu().numpy(), H.cpu().numpy()):.2e}")


# ------------------------------------------------------------------ 2. bit-exact composition
def composed(slk, f, s, z, R, gate):
    zm, H = f.ekf_linearize(FEAT, dev(params2(s)), s["m"])
    on_device(f, lambda zd, Rd: f.update_ekf(zd, zm, H.transpose(1, 2), Rd, gate=gate), z, R)


def model_update(f, s, z, R, gate, p=None):
    on_device(f, lambda zd, pd, Rd: f.update_ekf_model(zd, FEAT, pd, Rd, gate=gate), z, params2(s) if p is None else p, R)


@pytest.mark.parametrize("per_filter_R", [False, True], ids=["shared_R", "per_filter_R"])
@pytest.mark.parametrize("gate", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("k,m", [(8, 128), (8, 60), (9, 80), (8, 130)], ids=["tile-m128", "tile-m60", "general-N66", "general-m130"])
def test_update_ekf_model_is_linearize_plus_update_ekf(slk, k, m, gate, per_filter_R):
    s = ref.scenario(k, m, outliers=gate)
    R = sc.dense_noise(m, B=s["B"]) if per_filter_R else sc.dense_noise(m)
    fa, fb = slk.Msckf(s["mean"], s["P"]), slk.Msckf(s["mean"], s["P"])
    model_update(fa, s, s["z"], R, gate)
    composed(slk, fb, s, s["z"], R, gate)
    assert_same_state(fa, fb)
    assert not np.array_equal(fa.getPk(), s["P"]) or m == s["N"], "no filter took the update"
    # ... and the host route gives the same bits as the device route
    fc = slk.Msckf(s["mean"], s["P"])
    fc.update_ekf_model(s["z"], FEAT, params2(s), R, gate=gate)
    assert_same_state(fa, fc)


def test_update_ekf_model_after_lower_only_steps(slk):
    # three exact-shape UKF steps (k = 8, m = 8: P+ stored as its lower triangle only), no read-out in between
    k, m = 8, 64
    s = ref.scenario(k, m)
    u8 = sc.synthetic_msckf(s["B"], k, m=8, seed=0xE4F0 + k)
    fa, fb = slk.Msckf(s["mean"], s["P"]), slk.Msckf(s["mean"], s["P"])
    for f in (fa, fb):
        for _ in range(3):
            f.step(slk.PM_DELTA_POSE, u8["u"], u8["Q"], u8["z"], FEAT, u8["feat"].reshape(s["B"], -1), u8["R"])
    model_update(fa, s, s["z"], s["R"], True)
    composed(slk, fb, s, s["z"], s["R"], True)
    assert_same_state(fa, fb)
    assert (fa.status() & slk.ST_EKF_ROWS == 0).all(), "the EKF update was skipped"


# ------------------------------------------------------------------ 3. against the oracle
def check_against_oracle(s, res, gate):
    """Every filter against the oracle run of that filter alone on the numpy linearisation: equal status and outlier
    count; P and the mean (by boxminus) within TOL where the update was applied, the state bit-identical elsewhere."""
    st, out, P, M = res
    k, m = s["k"], s["m"]
    lay = o.layout(o.MULTI, k)
    zm, H = ref.linearize_np(s["mean"], s["feat"], k)
    applied, worst = 0, [0.0, 0.0]
    for b in range(s["B"]):
        if gate:                                              # no decision of ANY filter hinges on rounding
            d2 = ref.gate_d2(k, s["mean"][b], s["P"][b], s["z"][b], zm[b], H[b], s["R"])
            assert np.all(np.abs(d2[np.isfinite(d2)] - ref.CHI2) > 1e-6), (b, d2)
        rank, poses, ratio = ref.rank_premise(H[b])
        assert rank == 6 * poses and ratio > 1e-6, (b, rank, poses, ratio)
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        sto, no = r.update_ekf(s["z"][b], zm[b], H[b], s["R"], gate=gate)
        assert (st[b], out[b]) == (sto, no), (b, st[b], sto, out[b], no)
        if sto == 0 and no < m // 2:
            ep, em = rel(P[b], r.P), float(np.abs(o.boxminus(lay, M[b], r.mean)).max())
            assert ep <= TOL and em <= TOL, (b, ep, em)
            worst = [max(worst[0], ep), max(worst[1], em)]
            applied += 1
        else:
            assert np.array_equal(P[b], s["P"][b]) and np.array_equal(M[b], s["mean"][b]), b
    print(f"\nEKF from model k={k} m={m} gate={gate}: {applied} applied, worst relative error P {worst[0]:.2e}, mean {worst[1]:.2e}")
    return applied


@pytest.mark.parametrize("outliers", [False, True], ids=["clean", "outliers"])
@pytest.mark.parametrize("k,m", ref.SHAPES[:5], ids=IDS[:5])
def test_update_ekf_model_against_oracle(slk, k, m, outliers):
    s = ref.scenario(k, m, outliers=outliers)
    f = slk.Msckf(s["mean"], s["P"])
    f.update_ekf_model(s["z"], FEAT, params2(s), s["R"], gate=True)
    applied = check_against_oracle(s, (f.status(), f.outliers(), f.getPk(), f.muState()), True)
    if not outliers:
        assert applied == s["B"]
    elif m == s["N"]:                                         # fewer than N rows survive: SLK_ST_EKF_ROWS as from slk_update_ekf
        assert applied == 0 and (f.status() == slk.ST_EKF_ROWS).all()


# ------------------------------------------------------------------ 4. step and trajectory
class Traj:
    """T steps of a k = 8, m = 64 window: u, z and the landmarks vary per step."""

    def __init__(self, B=8, T=6, k=8, m=64, seed=0x57E9):
        rng = np.random.default_rng(seed)
        s = ref.scenario(k, m, B=B, seed=seed)
        self.s, self.B, self.T, self.k, self.m = s, B, T, k, m
        self.Q, self.R = s["Q"], s["R"]
        self.u = np.ascontiguousarray(np.broadcast_to(s["u"], (T, B, 13))).copy()
        self.u[:, :, 0:3] += rng.normal(0, 0.01, (T, B, 3))
        self.z = np.ascontiguousarray(s["z"][None] + rng.normal(0, 0.02, (T, B, m)))
        self.p = np.ascontiguousarray(np.broadcast_to(s["feat"], (T,) + s["feat"].shape)).copy()
        self.p[..., 0:3] += rng.normal(0, 0.01, (T, B, m // 2, 3))
        self.p = self.p.reshape(T, B, -1)
        self.truth = np.ascontiguousarray(np.broadcast_to(s["mean"], (T, B, s["Nq"]))).copy()

    def filt(self, slk):
        return slk.Msckf(self.s["mean"], self.s["P"])

    def single(self, slk, f, t, gate=True, device=False):
        def call(u, Q, z, p, R):
            f.step_ekf(slk.PM_DELTA_POSE, u, Q, z, FEAT, p, R, gate=gate)
        args = (self.u[t], self.Q, self.z[t], self.p[t], self.R)
        if device:
            on_device(f, call, *args)
        else:
            call(*args)


def test_step_ekf_is_predict_plus_update(slk):
    c = Traj()
    fa, fb = c.filt(slk), c.filt(slk)
    for t in range(2):
        c.single(slk, fa, t)
        fb.predict(slk.PM_DELTA_POSE, c.u[t], c.Q)
        fb.update_ekf_model(c.z[t], FEAT, c.p[t], c.R, gate=True)
        assert_same_state(fa, fb)
    assert (fa.status() == 0).all() and not np.array_equal(fa.muState(), c.s["mean"])


SCHEDULE = [-1, -1, 0, -1, -1, -1]


@pytest.mark.parametrize("slide", [None, 0, SCHEDULE], ids=["fixed_window", "slide0", "gated_schedule"])
@pytest.mark.parametrize("route", ["host", "device"])
def test_step_n_ekf_equals_single_steps(slk, route, slide):
    c = Traj()
    T, N = c.T, c.s["N"]
    # slide0: after every slide the landmarks no longer belong to the clones they index, so the gate is off there;
    # gated_schedule: one slide after step 2 with the gate on throughout and an outlier block in steps 1 and 4, so
    # that the outlier records before AND after the slide are non-zero
    gate = slide != 0
    if slide is SCHEDULE:
        c.z[[1, 4], :, 6] += 25.0
    sched = [slide] * T if slide == 0 else slide
    device = route == "device"
    d = dev if device else (lambda a: a)
    for nees_n in (6, N):
        fs, fn = c.filt(slk), c.filt(slk)
        means, outs, nees = [], [], []
        for t in range(T):
            c.single(slk, fs, t, gate=gate, device=device)
            if sched is not None and sched[t] >= 0:
                fs.drop_clone(sched[t])
                fs.clone_pose()
            means.append(fs.muState())
            outs.append(fs.outliers())
            nees.append(fs.nees(c.truth[t], 0, nees_n))
        rec = fn.step_n(slk.PM_DELTA_POSE, d(c.u), d(c.Q), d(c.z), FEAT, d(c.p), d(c.R), gate=gate, truth=d(c.truth),
                        nees_range=(0, nees_n), record_mean=True, record_outliers=True, slide=slide, update="ekf")
        if device:
            rec = {k: v.cpu().numpy() for k, v in rec.items()}
        assert_same_state(fs, fn)
        assert not np.array_equal(fs.muState(), c.s["mean"])
        if slide is SCHEDULE:
            print(f"\ngated schedule: outliers per step {np.stack(outs).sum(axis=1)}, status {fs.status()}")
            assert (np.stack(outs)[[1, 4]] >= 1).all()        # the records compared after the slide are not all zero
        else:
            assert (fs.status() & slk.ST_EKF_ROWS == 0).all()
        np.testing.assert_array_equal(rec["mean"], np.stack(means))
        np.testing.assert_array_equal(rec["outliers"], np.stack(outs))
        got, want = rec["nees"], np.stack(nees)
        if nees_n > 30:                                       # slk_nees's own kernel: bit-identical
            np.testing.assert_array_equal(got, want)
        else:                                                 # the one-wave register factorisation: 1e-10 (slk_step_n)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok]))


def test_ekf_trajectory_stays_on_the_oracle(slk):
    # 20 steps against the oracle looped on the CPU: 1e-9 is the single-update tolerance; over 20 steps the 1e-8 that
    # test_msckf_long_trajectory_stays_on_the_oracle allows the UKF over 30; equal summed outlier counts
    T, B, k, m = 20, 4, 8, 64
    c = Traj(B=B, T=T, k=k, m=m, seed=0x0DD5)
    c.z[::5, :, 6] += 25.0                                    # one outlier block every fifth step (62 >= N rows survive)
    f = c.filt(slk)
    rec = f.step_n(slk.PM_DELTA_POSE, c.u, c.Q, c.z, FEAT, c.p, c.R, gate=True, record_outliers=True, update="ekf")
    Pg, Mg = f.getPk(), f.muState()
    assert (f.status() == 0).all()
    lay = o.layout(o.MULTI, k)
    for b in range(B):
        r = o.Msckf(k, c.s["mean"][b], c.s["P"][b])
        total = 0
        for t in range(T):
            u = c.u[t, b]
            assert r.predict(o.pm_delta_pose(u[0:3], u[3:7], u[7:10], u[10:13]), c.Q) == 0
            feat = c.p[t, b].reshape(1, -1, 4)
            zm, H = ref.linearize_np(r.mean[None], feat, k)
            st, no = r.update_ekf(c.z[t, b], zm[0], H[0], c.R, gate=True)
            assert st == 0
            total += no
        assert total == int(rec["outliers"][:, b].astype(np.int64).sum()), (b, total)
        ep, em = rel(Pg[b], r.P), float(np.abs(o.boxminus(lay, Mg[b], r.mean)).max())
        print(f"\n20-step EKF trajectory, filter {b}: relative error P {ep:.2e}, mean {em:.2e}, outliers {total}")
        assert ep <= 1e-8 and em <= 1e-8, (b, ep, em)


# ------------------------------------------------------------------ 5. refusals and status
def refused(slk, call):
    with pytest.raises(slk.SlkError, match=r"code -1\b"):
        call()


def test_refusals_leave_the_filter_untouched(slk):
    k, m = 8, 64
    s = ref.scenario(k, m)
    p, z, R = params2(s), s["z"], s["R"]
    f = slk.Msckf(s["mean"], s["P"])
    before = state(f)
    M = slk.Msckf

    def every_call(model, p, z, R):
        mm = z.shape[-1]
        yield lambda: f.ekf_linearize(model, p, mm)
        yield lambda: f.update_ekf_model(z, model, p, R)
        yield lambda: f.step_ekf(slk.PM_DELTA_POSE, s["u"], s["Q"], z, model, p, R)
        yield lambda: f.step_n(slk.PM_DELTA_POSE, s["u"][None], s["Q"], z[None], model, None if p is None else p[None], R,
                               update="ekf")

    dummy = np.zeros((s["B"], 4 * m))
    for model in (POSE, VO, EXT):
        for call in every_call(model, dummy, z, R):
            refused(slk, call)
    for mm in (s["N"] - 2, 61, 514):                          # m < N, odd m, m > 512
        zz, RR, pp = np.zeros((s["B"], mm)), np.eye(mm), np.zeros((s["B"], 4 * mm))
        pp[:, 2::4] = 5.0
        for call in every_call(FEAT, pp, zz, RR):
            refused(slk, call)
    for bad in (k + 1, -1, np.nan):                           # host-resident pose indices
        pb = p.copy()
        pb[2, 4 * 7 + 3] = bad
        for call in every_call(FEAT, pb, z, R):
            refused(slk, call)
    lib = slk.load_library()                                   # a short p_stride (the wrapper cannot express one)
    pc, zc, Rc = np.ascontiguousarray(p), np.ascontiguousarray(z), np.ascontiguousarray(R)
    zm, H = np.empty((s["B"], m)), np.empty((s["B"], s["N"], m))
    assert lib.slk_ekf_linearize(f._h, FEAT, pc.ctypes.data, 2 * m - 1, m, zm.ctypes.data, H.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_update_ekf_model(f._h, FEAT, pc.ctypes.data, 2 * m - 1, zc.ctypes.data, m, Rc.ctypes.data, 0, 1, slk.HOST) == slk.E_INVALID
    # step_n's own refusals on the EKF kind: a slide index outside -1 .. k - 1, a record without its truth range
    refused(slk, lambda: f.step_n(slk.PM_DELTA_POSE, s["u"][None], s["Q"], z[None], FEAT, p[None], R, slide=k, update="ekf"))
    refused(slk, lambda: f.step_n(slk.PM_DELTA_POSE, s["u"][None], s["Q"], z[None], FEAT, p[None], R, truth=s["mean"][None],
                                  nees_range=(0, s["N"] + 1), update="ekf"))
    refused(slk, lambda: f.step_n(99, s["u"][None], s["Q"], z[None], FEAT, p[None], R, update="ekf"))
    for x, y in zip(before, state(f)):
        np.testing.assert_array_equal(x, y)
    # a Usckf handle
    su = sc.synthetic_usckf(2)
    fu = slk.Usckf(mean=su["mean"], P=su["P"], nfk=3, nfkl=9)
    bu = (fu.muState(), fu.PkAugmentedState(), fu.status())
    mu = 48
    refused(slk, lambda: M.ekf_linearize(fu, FEAT, np.zeros((2, 2 * mu)), mu))
    refused(slk, lambda: M.update_ekf_model(fu, np.zeros((2, mu)), FEAT, np.zeros((2, 2 * mu)), np.eye(mu)))
    refused(slk, lambda: M.step_ekf(fu, slk.PM_CONST_VELOCITY, su["u"], su["Q"], np.zeros((2, mu)), FEAT, np.zeros((2, 2 * mu)), np.eye(mu)))
    refused(slk, lambda: fu.step_n(slk.PM_CONST_VELOCITY, su["u"][None], su["Q"], np.zeros((1, 2, mu)), FEAT,
                                   np.zeros((1, 2, 2 * mu)), np.eye(mu), update="ekf"))
    for x, y in zip(bu, (fu.muState(), fu.PkAugmentedState(), fu.status())):
        np.testing.assert_array_equal(x, y)


def test_step_n_ekf_rejects_bad_calls(slk):
    """Each of slk_step_n's own refusals (tests/test_gpu_trajectory.py: test_step_n_rejects_bad_calls) and those of the
    EKF step kind, sent to slk_step_n_ekf through a raw slk_traj with slide NULL and non-NULL, and the argument checks of
    slk_step_ekf / slk_update_ekf_model / slk_ekf_linearize: SLK_E_INVALID, the filter bit-unchanged, every time."""
    lib = slk.load_library()
    c = Traj(B=4, T=3)
    T, B, k, m, N, Nq = c.T, c.B, c.k, c.m, c.s["N"], c.s["Nq"]
    f = c.filt(slk)
    c.single(slk, f, 0)                                        # a state that a stray launch would change
    before = state(f)
    Q, R = np.ascontiguousarray(c.Q.T), np.ascontiguousarray(c.R.T)
    Rb = np.ascontiguousarray(np.broadcast_to(R, (B, m, m)))
    npar = 2 * m
    truth = np.ascontiguousarray(c.truth)
    nees = np.empty((T, B))
    p_bad = c.p.copy()
    p_bad[2, 1, 4 * 3 + 3] = k + 1                            # a pose index out of range in the LAST step only
    p_nan = c.p.copy()
    p_nan[1, 0, 3] = np.nan
    z66, R66, p66 = np.zeros((T, B, 66)), np.eye(66) * 0.01, np.zeros((T, B, 4 * 66))
    ok_slide = np.array([-1, 0, -1], dtype=np.int32)

    def traj(**kw):
        t = slk.Traj()
        t.T, t.pmodel, t.u, t.u_stride, t.u_tstride = T, slk.PM_DELTA_POSE, c.u.ctypes.data, 13, B * 13
        t.Q, t.q_stride, t.q_tstride = Q.ctypes.data, 0, 0
        t.mmodel, t.params, t.p_stride, t.p_tstride = FEAT, c.p.ctypes.data, npar, B * npar
        t.z, t.m, t.z_tstride = c.z.ctypes.data, m, B * m
        t.R, t.r_stride, t.r_tstride = R.ctypes.data, 0, 0
        t.gate = 1
        for key, v in kw.items():
            setattr(t, key, v)
        return t

    def m_rows(mm):
        return traj(z=z66.ctypes.data, m=mm, z_tstride=B * 66, R=R66.ctypes.data, params=p66.ctypes.data, p_stride=4 * 66,
                    p_tstride=B * 4 * 66)

    bad = {
        # slk_step_n's own list
        "T0": traj(T=0),
        "null-z": traj(z=None),
        "nees-without-truth": traj(nees_hist=nees.ctypes.data),
        "short-z-tstride": traj(z_tstride=B * m - 1),
        "negative-u-tstride": traj(u_tstride=-13 * B),
        "external-model": traj(mmodel=slk.MODEL_EXTERNAL),
        "unknown-where": None,
        "bad-nees-range": traj(truth=truth.ctypes.data, truth_tstride=B * Nq, nees_t0=N - 5, nees_n=6, nees_hist=nees.ctypes.data),
        "short-truth-tstride": traj(truth=truth.ctypes.data, truth_tstride=B * Nq - 1, nees_t0=0, nees_n=6, nees_hist=nees.ctypes.data),
        "null-u": traj(u=None),
        "null-Q": traj(Q=None),
        "short-u-stride": traj(u_stride=12),
        "short-q-stride": traj(q_stride=143),
        "unknown-process-model": traj(pmodel=99),
        "short-q-tstride": traj(q_tstride=143),
        "short-r-tstride": traj(r_tstride=m * m - 1),
        # the measurement side of the EKF step kind
        "null-R": traj(R=None),
        "short-r-stride": traj(R=Rb.ctypes.data, r_stride=m * m - 1),
        "null-params": traj(params=None),
        "short-p-stride": traj(p_stride=npar - 1),
        "short-p-tstride": traj(p_tstride=B * npar - 1),
        "pose-position-model": traj(mmodel=POSE),
        "vo-relative-model": traj(mmodel=VO),
        "rows-below-N": m_rows(N - 2),
        "odd-rows": m_rows(61),
        "rows-above-512": traj(m=514),
        "pose-index-k+1-in-the-last-step": traj(params=p_bad.ctypes.data),
        "pose-index-nan": traj(params=p_nan.ctypes.data),
    }
    for name, t in bad.items():
        where = slk.HOST
        if t is None:
            t, where = traj(), 2
        for sl in (None, ok_slide.ctypes.data):
            assert lib.slk_step_n_ekf(f._h, C.byref(t), sl, where) == slk.E_INVALID, name
            for x, y in zip(before, state(f)):
                np.testing.assert_array_equal(x, y, err_msg=name)
    for sched in ([-1, k, -1], [-2, -1, -1]):                  # a schedule entry outside -1 .. k - 1
        sl = np.array(sched, dtype=np.int32)
        assert lib.slk_step_n_ekf(f._h, C.byref(traj()), sl.ctypes.data, slk.HOST) == slk.E_INVALID, sched
    # the single calls: (u, u_stride, Q, q_stride, model, params, p_stride, z, m, R, r_stride, where)
    u0, z0, p0 = c.u[0], c.z[0], c.p[0]
    good = dict(pm=slk.PM_DELTA_POSE, u=u0.ctypes.data, us=13, Q=Q.ctypes.data, qs=0, mm=FEAT, p=p0.ctypes.data, ps=npar,
                z=z0.ctypes.data, m=m, R=R.ctypes.data, rs=0, where=slk.HOST)
    p0bad = p_bad[2]
    single = {
        "short-p-stride": dict(ps=npar - 1), "null-params": dict(p=None), "null-z": dict(z=None), "null-R": dict(R=None),
        "short-r-stride": dict(R=Rb.ctypes.data, rs=m * m - 1), "unknown-where": dict(where=2), "odd-rows": dict(m=m - 1),
        "rows-below-N": dict(m=N - 2), "rows-above-512": dict(m=514), "external-model": dict(mm=slk.MODEL_EXTERNAL),
        "pose-position-model": dict(mm=POSE), "pose-index-k+1": dict(p=p0bad.ctypes.data),
    }
    step_only = {"null-u": dict(u=None), "null-Q": dict(Q=None), "short-u-stride": dict(us=12), "short-q-stride": dict(qs=143),
                 "unknown-process-model": dict(pm=99)}
    zm, H = np.empty((B, m)), np.empty((B, N, m))
    for name, kw in list(single.items()) + list(step_only.items()):
        a = dict(good, **kw)
        assert lib.slk_step_ekf(f._h, a["pm"], a["u"], a["us"], a["Q"], a["qs"], a["mm"], a["p"], a["ps"], a["z"], a["m"],
                                a["R"], a["rs"], 1, a["where"]) == slk.E_INVALID, name
        if name in single:
            assert lib.slk_update_ekf_model(f._h, a["mm"], a["p"], a["ps"], a["z"], a["m"], a["R"], a["rs"], 1,
                                            a["where"]) == slk.E_INVALID, name
            if name not in ("null-z", "null-R", "short-r-stride"):
                assert lib.slk_ekf_linearize(f._h, a["mm"], a["p"], a["ps"], a["m"], zm.ctypes.data, H.ctypes.data,
                                             a["where"]) == slk.E_INVALID, name
        for x, y in zip(before, state(f)):
            np.testing.assert_array_equal(x, y, err_msg=name)
    assert lib.slk_ekf_linearize(f._h, FEAT, p0.ctypes.data, npar, m, None, H.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_ekf_linearize(f._h, FEAT, p0.ctypes.data, npar, m, zm.ctypes.data, None, slk.HOST) == slk.E_INVALID
    for x, y in zip(before, state(f)):
        np.testing.assert_array_equal(x, y)
    # the unmodified calls are accepted
    assert lib.slk_step_n_ekf(f._h, C.byref(traj()), ok_slide.ctypes.data, slk.HOST) == 0
    a = good
    assert lib.slk_step_ekf(f._h, a["pm"], a["u"], a["us"], a["Q"], a["qs"], a["mm"], a["p"], a["ps"], a["z"], a["m"], a["R"],
                            a["rs"], 1, a["where"]) == 0
    assert not np.array_equal(f.muState(), before[0])


@pytest.mark.parametrize("k,m", [(8, 64), (9, 80)], ids=["tile", "general"])
@pytest.mark.parametrize("bad", ["k+1", "-1", "nan"])
def test_bad_device_index_skips_that_filter_only(slk, k, m, bad):
    s = ref.scenario(k, m)
    p = params2(s)
    pb = p.copy()
    pb[1, 4 * 5 + 3] = {"k+1": k + 1, "-1": -1.0, "nan": np.nan}[bad]
    good, f = slk.Msckf(s["mean"], s["P"]), slk.Msckf(s["mean"], s["P"])
    model_update(good, s, s["z"], s["R"], True, p)
    model_update(f, s, s["z"], s["R"], True, pb)
    Mg, Pg, stg, og = state(good)
    Mf, Pf, stf, of = state(f)
    assert stf[1] == slk.ST_BAD_INDEX and of[1] == 0
    assert np.array_equal(Mf[1], s["mean"][1]) and np.array_equal(Pf[1], s["P"][1])
    for b in (0, 2, 3):
        assert stf[b] == stg[b] == 0 and of[b] == og[b]
        assert np.array_equal(Mf[b], Mg[b]) and np.array_equal(Pf[b], Pg[b])
        assert not np.array_equal(Pf[b], s["P"][b])
    # the public linearisation reports the same filter and marks its rows
    f2 = slk.Msckf(s["mean"], s["P"])
    zm, H = f2.ekf_linearize(FEAT, dev(pb), m)
    zm, H = zm.cpu().numpy(), H.cpu().numpy()
    assert list(f2.status()) == [0, slk.ST_BAD_INDEX, 0, 0]
    assert np.isnan(zm[1]).all() and np.isnan(H[1]).all() and not np.isnan(zm[[0, 2, 3]]).any() and not np.isnan(H[[0, 2, 3]]).any()
    assert np.array_equal(f2.muState(), s["mean"]) and np.array_equal(f2.getPk(), s["P"])
