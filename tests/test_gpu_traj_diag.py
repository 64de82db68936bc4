"""Per-step consistency records of trajectories (slk_step_n_diag / step_n(diag=...)).

* everything a call without records returns is bit-identical with them (the records are extra work beside the step);
* sigma_hist[t] is slk_get_sigma after t + 1 single steps on a twin, bit for bit;
* nis_hist[t] / logdet_hist[t] against single calls: a fresh twin is set to the state before step t (from a third handle
  advanced with slk_step and read by slk_get_state), then slk_predict with step t's inputs and slk_nis with step t's
  measurement.  Restarting the twin at every t keeps the rounding differences between the fused step and predict +
  update from accumulating; the shadow of a step runs the same launches as the twin, so the records are also asserted
  bit for bit.  Tolerance (rtol 1e-9 on nis, atol 1e-9 * m on logdet) and the condition cond(S) <= 1e4 as in
  tests/test_gpu_nis.py, S being what slk_update_innovation emits on the twin;
* the EKF step kind takes sigma records only; d == NULL and an all-NULL d are the existing entry points;
* a statistical sanity check of the NIS of a consistent Monte-Carlo batch.
"""
import ctypes as C

import numpy as np
import pytest

import scenarios as sc
import test_gpu_trajectory as tj
import nis_support as tn

pytestmark = pytest.mark.gpu
FEAT, POSE, VO = 2, 3, 1
Case = tj.Case


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def colmajor(M):
    return M.T if M.ndim == 2 else np.transpose(M, (0, 2, 1))


def run_n(c, f, slide=None, diag=(), device=False, truth=None):
    kw = dict(gate=c.gate, record_mean=True, record_outliers=True, slide=slide, diag=diag)
    if device:
        p = c.params_t()
        rec = f.step_n(c.pm, dev(c.u), dev(colmajor(c.Q)), dev(c.z), c.model, None if p is None else dev(p), dev(colmajor(c.R)),
                       truth=dev(truth), **kw)
        return {k: v.cpu().numpy() for k, v in rec.items()}
    return f.step_n(c.pm, c.u, c.Q, c.z, c.model, c.params_t(), c.R, truth=truth, **kw)


def single(c, f, t, sched):
    c.single(f, t)
    if sched is not None and sched[t] >= 0:
        f.slide(int(sched[t]))


def set_twin(c, slk, mean, P):
    if c.kind == "msckf":
        return slk.Msckf(mean, P)
    return slk.Usckf(mean=mean, P=P, nfk=c.nfk, nfkl=c.nfkl)


CASES = [
    ("msckf-k8-m8-fast", dict(kind="msckf", B=8, k=8, m=8), None),
    ("msckf-k8-m8-fast-slide", dict(kind="msckf", B=8, k=8, m=8), [0, -1, 3, -1, 7, 0]),
    ("msckf-k2-m4", dict(kind="msckf", B=8, k=2, m=4), None),
    ("msckf-k2-m4-slide", dict(kind="msckf", B=8, k=2, m=4), [-1, 1, -1, 0, 0, -1]),
    ("msckf-k12-m8", dict(kind="msckf", B=8, k=12, m=8), None),
    ("msckf-k12-m8-slide", dict(kind="msckf", B=8, k=12, m=8), [11, -1, -1, 0, -1, 5]),
    ("usckf-N48-m3", dict(kind="usckf", B=8, nfk=3, nfkl=9, m=3, model=VO), None),
    ("usckf-N48-wide-m40", dict(kind="usckf", B=8, nfk=3, nfkl=9, m=40, model=FEAT), None),
]
T = 6


# ------------------------------------------------------------------ 6. trajectory records
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("name,spec,sched", CASES, ids=[c[0] for c in CASES])
def test_records_beside_the_steps(slk, name, spec, sched, route):
    c = Case(T=T, **spec)
    device = route == "device"
    sl = None if sched is None else np.array(sched, dtype=np.int32)
    truth = np.repeat(c.s["mean"][None], T, axis=0)
    # the same call without and with records: everything it returned before is bit-identical
    fp, fd = c.filt(slk), c.filt(slk)
    plain = run_n(c, fp, sl, device=device, truth=truth)
    rec = run_n(c, fd, sl, diag=("nis", "logdet", "sigma"), device=device, truth=truth)
    tj.assert_same_state(fp, fd)
    for key in ("mean", "outliers", "nees"):
        np.testing.assert_array_equal(rec[key], plain[key], err_msg=key)
    assert rec["nis"].shape == (T, c.B) and rec["logdet"].shape == (T, c.B) and rec["sigma"].shape == (T, c.B, fp.N)
    # single records alone are the same numbers
    fo = c.filt(slk)
    only = run_n(c, fo, sl, diag=("logdet",), device=device)
    assert set(only) == {"mean", "outliers", "logdet"}
    np.testing.assert_array_equal(only["logdet"], rec["logdet"])
    tj.assert_same_state(fp, fo)
    # single steps: sigma after each, and the state before each for the NIS twins
    fs = c.filt(slk)
    for t in range(T):
        m0, P0 = fs.muState(), fs._getP()
        tw = set_twin(c, slk, m0, P0)
        tw.predict(c.pm, c.u[t], c.Q)
        want_n, want_ld = tw.nis(c.z[t], c.model, c.params, c.R, logdet=True)
        rc, S, _ = tn.innovation(slk, tw, c.model, c.params, c.z[t], c.R)
        assert rc == 0
        for b in range(c.B):
            cond = np.linalg.cond(S[b])
            assert cond <= tn.COND_MAX, (name, t, b, "cond(S)", cond)
        tn.assert_stats(rec["nis"][t], rec["logdet"][t], want_n, want_ld, c.m, (name, route, t))
        # (stricter than the tolerance asked for: the shadow runs the twin's launches on a copy of the same numbers)
        np.testing.assert_array_equal(rec["nis"][t], want_n, err_msg=f"nis of step {t}")
        np.testing.assert_array_equal(rec["logdet"][t], want_ld, err_msg=f"logdet of step {t}")
        single(c, fs, t, sl)
        np.testing.assert_array_equal(rec["sigma"][t], fs.sigma(), err_msg=f"sigma after step {t}")
    tj.assert_same_state(fs, fd)
    assert np.isfinite(rec["nis"]).all() and (rec["nis"] > 0).all()


def test_a_failing_filter_records_nan(slk):
    """An indefinite P for filter 5: its steps are skipped with SLK_ST_LLT_FAIL as without records, its NIS records are
    NaN, the other filters' records are those of a batch without it."""
    c = Case(T=4, kind="msckf", B=8, k=2, m=4)
    P = c.s["P"].copy()
    P[5] = -P[5]
    fa, fb, fc = c.filt(slk, P), c.filt(slk, P), c.filt(slk)
    plain = run_n(c, fa)
    rec = run_n(c, fb, diag=("nis", "logdet", "sigma"))
    good = run_n(c, fc, diag=("nis", "logdet"))
    tj.assert_same_state(fa, fb)
    np.testing.assert_array_equal(rec["mean"], plain["mean"])
    assert fb.status()[5] & slk.ST_LLT_FAIL
    assert np.isnan(rec["nis"][:, 5]).all() and np.isnan(rec["logdet"][:, 5]).all()
    assert np.isnan(rec["sigma"][:, 5]).any()                    # (negative diagonal entries)
    keep = np.arange(c.B) != 5
    np.testing.assert_array_equal(rec["nis"][:, keep], good["nis"][:, keep])
    np.testing.assert_array_equal(rec["logdet"][:, keep], good["logdet"][:, keep])


def traj_struct(slk, c, keep):
    """struct slk_traj of the host route for a Case (the arrays are kept alive in `keep`)."""
    tr = slk.Traj()
    p = np.ascontiguousarray(c.params_t())
    Q, R = np.ascontiguousarray(c.Q.T), np.ascontiguousarray(c.R.T)
    keep += [p, Q, R]
    tr.T = c.T
    tr.pmodel, tr.u, tr.u_stride, tr.u_tstride = c.pm, c.u.ctypes.data, c.u.shape[2], c.u.shape[1] * c.u.shape[2]
    tr.Q, tr.q_stride, tr.q_tstride = Q.ctypes.data, 0, 0
    tr.mmodel, tr.params, tr.p_stride, tr.p_tstride = c.model, p.ctypes.data, p.shape[2], p.shape[1] * p.shape[2]
    tr.z, tr.m, tr.z_tstride = c.z.ctypes.data, c.m, c.B * c.m
    tr.R, tr.r_stride, tr.r_tstride = R.ctypes.data, 0, 0
    tr.gate = c.gate
    return tr


def test_null_records_are_the_existing_entry_points(slk):
    """d == NULL and an all-NULL d: bit-identical to slk_step_n_slide / slk_step_n_ekf."""
    lib = slk.load_library()
    c = Case(T=5, kind="msckf", B=8, k=8, m=8)
    sl = np.array([-1, 0, -1, 2, -1], dtype=np.int32)
    keep = []
    tr = traj_struct(slk, c, keep)
    ref = c.filt(slk)
    assert lib.slk_step_n_slide(ref._h, C.byref(tr), sl.ctypes.data, slk.HOST) == 0
    for d in (None, C.byref(slk.TrajDiag())):
        f = c.filt(slk)
        assert lib.slk_step_n_diag(f._h, C.byref(tr), sl.ctypes.data, 0, d, slk.HOST) == 0
        tj.assert_same_state(ref, f)
    import test_gpu_ekf_model as em
    e = em.Traj()
    ref = e.filt(slk)
    ref.step_n(slk.PM_DELTA_POSE, e.u, e.Q, e.z, FEAT, e.p, e.R, gate=True, update="ekf")
    er = slk.Traj()
    Q, R = np.ascontiguousarray(e.Q.T), np.ascontiguousarray(colmajor(e.R))
    er.T = e.T
    er.pmodel, er.u, er.u_stride, er.u_tstride = slk.PM_DELTA_POSE, e.u.ctypes.data, 13, e.B * 13
    er.Q, er.q_stride, er.q_tstride = Q.ctypes.data, 0, 0
    er.mmodel, er.params, er.p_stride, er.p_tstride = FEAT, e.p.ctypes.data, e.p.shape[2], e.B * e.p.shape[2]
    er.z, er.m, er.z_tstride = e.z.ctypes.data, e.m, e.B * e.m
    er.R, er.r_stride, er.r_tstride = R.ctypes.data, (0 if e.R.ndim == 2 else e.m * e.m), 0
    er.gate = 1
    for d in (None, C.byref(slk.TrajDiag())):
        f = e.filt(slk)
        assert lib.slk_step_n_diag(f._h, C.byref(er), None, 1, d, slk.HOST) == 0
        em.assert_same_state(ref, f)


def test_ekf_steps_record_sigma_only(slk):
    """ekf != 0 with nis_hist or logdet_hist: SLK_E_INVALID, the filter bit-identical; with sigma_hist only: the records of
    the single-step loop, the state that of the call without records."""
    import test_gpu_ekf_model as em
    e = em.Traj()
    f = e.filt(slk)
    before = em.state(f)
    for diag in (("nis",), ("logdet",), ("nis", "logdet", "sigma")):
        with pytest.raises(slk.SlkError, match="code -1"):
            f.step_n(slk.PM_DELTA_POSE, e.u, e.Q, e.z, FEAT, e.p, e.R, gate=True, update="ekf", diag=diag)
    for x, y in zip(before, em.state(f)):
        np.testing.assert_array_equal(x, y)
    sched = np.array(em.SCHEDULE, dtype=np.int32)
    rec = f.step_n(slk.PM_DELTA_POSE, e.u, e.Q, e.z, FEAT, e.p, e.R, gate=True, update="ekf", slide=sched, diag=("sigma",),
                   record_mean=True)
    plain = e.filt(slk)
    pr = plain.step_n(slk.PM_DELTA_POSE, e.u, e.Q, e.z, FEAT, e.p, e.R, gate=True, update="ekf", slide=sched, record_mean=True)
    em.assert_same_state(plain, f)
    np.testing.assert_array_equal(rec["mean"], pr["mean"])
    fs = e.filt(slk)
    for t in range(e.T):
        e.single(slk, fs, t)
        if sched[t] >= 0:
            fs.slide(int(sched[t]))
        np.testing.assert_array_equal(rec["sigma"][t], fs.sigma(), err_msg=f"sigma after step {t}")


def test_msckf_wide_rows_and_external_are_refused(slk):
    """SLK_MODEL_EXTERNAL and Msckf m > 32 are refused as in slk_step_n, the filter untouched."""
    lib = slk.load_library()
    c = Case(T=3, kind="msckf", B=4, k=2, m=4)
    keep = []
    tr = traj_struct(slk, c, keep)
    f = c.filt(slk)
    before = tj.state(f)
    nis = np.full((3, 4), -7.0)
    d = slk.TrajDiag(nis.ctypes.data, None, None)
    tr.mmodel = slk.MODEL_EXTERNAL
    assert lib.slk_step_n_diag(f._h, C.byref(tr), None, 0, C.byref(d), slk.HOST) == slk.E_INVALID
    tr.mmodel, tr.m = FEAT, 34
    assert lib.slk_step_n_diag(f._h, C.byref(tr), None, 0, C.byref(d), slk.HOST) == slk.E_INVALID
    assert (nis == -7.0).all()
    for x, y in zip(before, tj.state(f)):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ 8. a statistical sanity check
def monte_carlo(B, T, k, m, seed):
    """A consistent batch: every filter starts at a truth state perturbed by a draw from its own P; the truth moves by the
    filter's own process model with process noise drawn from Q (on the 12 tangent components of the current state), and
    every measurement is h(truth) plus a draw from the R the filter is given."""
    from oracle import oracle as o
    from oracle import np_check as npc
    rng = np.random.default_rng(seed)
    s = sc.synthetic_msckf(B, k, m=m, seed=seed)
    N, lay = s["N"], o.layout(o.MULTI, k)
    R = 0.01 * np.eye(m)
    Q = np.asarray(s["Q"], dtype=np.float64).reshape(12, 12)
    Lq, Lr = np.linalg.cholesky(Q), np.linalg.cholesky(R)
    truth = np.empty_like(s["mean"])
    for b in range(B):
        Lp = np.linalg.cholesky(s["P"][b].reshape(N, N))
        truth[b] = o.boxplus(lay, s["mean"][b], Lp @ rng.normal(0, 1, N))
    single = o.layout(o.MULTI, 0)
    z = np.empty((T, B, m))
    for t in range(T):
        for b in range(B):
            ub = s["u"][b]
            x13 = npc.pm_delta_pose(truth[b, :13], ub[0:3], ub[3:7], ub[7:10], ub[10:13])
            truth[b, :13] = o.boxplus(single, x13, Lq @ rng.normal(0, 1, 12))
            z[t, b] = npc.mm_feature_proj(truth[b], s["feat"][b]) + Lr @ rng.normal(0, 1, m)
    return s, R, z


def test_nis_of_a_consistent_batch_is_chi_square(slk):
    """B = 2048 Msckf filters, k = 4, m = 8, 20 steps, ungated, measurements drawn with the R the filter is given: the
    mean of nis_hist over B and t lies within m +- 3.29 sqrt(2 m / (B T)) (the two-sided 99.9 % interval of a chi-square
    with B T m degrees of freedom divided by B T, normal approximation).

    The seed was kept after running the same draw through the numpy reference on the CPU first (the oracle's Msckf on a
    subsample of 64 filters, nis = nu @ solve(S, nu) from its sigma points): the reference's mean NIS lies inside its own
    interval m +- 3.29 sqrt(2 m / (64 T)) for this seed (8.067 in [7.632, 8.368]).  The unscented transform of the projection model is not exactly
    Gaussian-consistent, so the check is a sanity check of scale, not a proof of the kernel (tests/test_gpu_nis.py is)."""
    B, Tn, k, m = 2048, 20, 4, 8
    s, R, z = monte_carlo(B, Tn, k, m, seed=0x2048)
    f = slk.Msckf(s["mean"], s["P"])
    u = np.broadcast_to(s["u"], (Tn,) + s["u"].shape)
    p = np.broadcast_to(s["feat"].reshape(B, -1), (Tn, B, 2 * m))
    rec = f.step_n(slk.PM_DELTA_POSE, u, s["Q"], z, FEAT, p, R, gate=0, diag=("nis",))
    assert (f.status() == 0).all()
    mean_nis = float(rec["nis"].mean())
    half = 3.29 * np.sqrt(2.0 * m / (B * Tn))
    print("mean NIS", mean_nis, "interval", m - half, m + half)
    assert m - half <= mean_nis <= m + half, (mean_nis, m - half, m + half)
