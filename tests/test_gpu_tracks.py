"""Msckf feature-track update (slk_track_linearize, slk_update_tracks, slk_step_tracks): the device triangulation and
null-space marginalisation against the numpy twin (tracks_ref.py) in basis-independent quantities, every flag, bit-exact
composition with slk_update_ekf on both of its kernels, the update against the CPU oracle run one filter at a time, and
every refusal.  Run with `pytest -m gpu` on an MI355X (`-s` prints the errors seen)."""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
import tracks_ref as tr

pytestmark = pytest.mark.gpu

TOL = 1e-9                                    # the tolerance tests/test_gpu_ekf.py uses for this update
FEAT = 2


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def state(f):
    return f.muState(), f.getPk(), f.status(), f.outliers()


def assert_same_state(fa, fb):
    for x, y in zip(state(fa), state(fb)):
        np.testing.assert_array_equal(x, y)


def filt(slk, s):
    return slk.Msckf(s["mean"], s["P"])


def observed_columns(track, N):
    """the columns of the poses a track observes"""
    cols = np.zeros(N, dtype=bool)
    for c in track[:, 0]:
        if c >= 0:
            tp = tr.pose_offsets(int(c))[1]
            cols[tp:tp + 6] = True
    return cols


def check_linearisation(s, r, H, feat, chi2=None, twin=None):
    """feat against the twin at TOL; H^T H, H^T r, r^T r per filter at TOL of their largest entry; exact +0.0 outside each
    row's observed poses, in the rows of tracks that are not used and in the padding rows; no NaN anywhere."""
    B, J, M, m, N = s["B"], s["J"], s["M"], s["m"], s["N"]
    nr = 2 * M - 3
    rt, Ht, ft, gam = twin if twin is not None else tr.linearize_batch(s, chi2)
    assert r.shape == (B, m) and H.shape == (B, m, N) and feat.shape == (B, J, 4)
    assert not np.isnan(r).any() and not np.isnan(H).any(), "a store is missing"
    if chi2 is not None:                                      # no gate decision hinges on rounding
        for b in range(B):
            for j in range(J):
                if np.isfinite(gam[b, j]):
                    thr = chi2[2 * int((s["tracks"][b, j, :, 0] >= 0).sum()) - 3]
                    assert abs(gam[b, j] - thr) > 1e-6 * thr, (b, j, gam[b, j], thr)
    np.testing.assert_array_equal(feat[..., 3], ft[..., 3])
    worst = [0.0, 0.0]
    rbits, Hbits = np.ascontiguousarray(r).view(np.uint64), np.ascontiguousarray(H).view(np.uint64)
    for b in range(B):
        for j in range(J):
            flag, rows = int(ft[b, j, 3]), slice(j * nr, (j + 1) * nr)
            if flag in (1, -2):
                e = rel(feat[b, j, :3], ft[b, j, :3])
                assert e <= TOL, (b, j, e)
                worst[0] = max(worst[0], e)
            elif flag == 0:
                assert (np.ascontiguousarray(feat[b, j, :3]).view(np.uint64) == 0).all()
            else:
                assert np.isnan(feat[b, j, :3]).all()
            if flag == 1:
                assert (Hbits[b, rows][:, ~observed_columns(s["tracks"][b, j], N)] == 0).all(), (b, j)
                assert np.abs(H[b, rows]).max() > 0
            else:
                assert (Hbits[b, rows] == 0).all() and (rbits[b, rows] == 0).all(), (b, j, flag)
        assert (Hbits[b, J * nr:] == 0).all() and (rbits[b, J * nr:] == 0).all(), "padding rows"
        for got, want in ((H[b].T @ H[b], Ht[b].T @ Ht[b]), (H[b].T @ r[b], Ht[b].T @ rt[b]), (r[b] @ r[b], rt[b] @ rt[b])):
            e = float(np.abs(got - want).max() / max(1e-300, np.abs(want).max()))
            assert e <= TOL, (b, e)
            worst[1] = max(worst[1], e)
    return worst


# ------------------------------------------------------------------ 1. the linearisation
@pytest.mark.parametrize("shared", [False, True], ids=["per_filter", "shared"])
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("k,M,J,m", tr.SHAPES, ids=tr.IDS)
def test_linearisation(slk, k, M, J, m, route, shared):
    s = tr.scenario(k, M, J, m, shared=shared)
    chi2 = tr.CHI2_95[:2 * M - 2]
    f = filt(slk, s)
    before = state(f)
    t = s["tracks"][0] if shared else s["tracks"]
    if route == "device":
        import torch
        r, H, feat = f.track_linearize(dev(t), s["sigma"], m, chi2=chi2)
        for x in (r, H, feat):                                # a second call into NaN-filled buffers: every entry is stored
            x.fill_(float("nan"))
        torch.cuda.synchronize()
        lib, td, sd, cd = slk.load_library(), dev(t), dev(np.array([s["sigma"]])), dev(chi2)
        assert lib.slk_track_linearize(f._h, td.data_ptr(), 0 if shared else 3 * J * M, J, M, sd.data_ptr(), 0, cd.data_ptr(), m,
                                       r.data_ptr(), H.transpose(1, 2).data_ptr(), feat.data_ptr(), slk.DEVICE) == 0
        f.sync()
        r, H, feat = r.cpu().numpy(), H.cpu().numpy(), feat.cpu().numpy()
    else:
        r, H, feat = f.track_linearize(t, s["sigma"], m, chi2=chi2)
    w = check_linearisation(s, r, H, feat, chi2)
    print(f"\ntracks k={k} M={M} J={J} m={m} {route}: worst relative error X {w[0]:.2e}, H^T H / H^T r / r^T r {w[1]:.2e}, "
          f"flags {np.unique(feat[..., 3]).tolist()}")
    for x, y in zip(before, state(f)):                        # the filter is not modified
        np.testing.assert_array_equal(x, y)


def test_linearisation_without_gate_and_per_filter_sigma(slk):
    k, M, J, m = tr.SHAPES[3]
    s = tr.scenario(k, M, J, m)
    f = filt(slk, s)
    r, H, feat = f.track_linearize(s["tracks"], np.full(s["B"], s["sigma"]), m)
    check_linearisation(s, r, H, feat)
    r2, H2, feat2 = f.track_linearize(s["tracks"], s["sigma"], m)
    np.testing.assert_array_equal(r, r2)
    np.testing.assert_array_equal(H, H2)
    np.testing.assert_array_equal(feat, feat2)


# ------------------------------------------------------------------ 2. flags
def test_flags(slk):
    s, s2, b = tr.flag_scenario()
    M, m = s["M"], s["m"]
    nr = 2 * M - 3
    chi2 = tr.CHI2_95[:2 * M - 2]
    twin = tr.linearize_batch(s2, chi2)
    assert twin[2][b, :5, 3].tolist() == [0, 0, -1, -1, -2], (twin[2][b, :5, 3], twin[3][b])
    r0, H0, feat0 = filt(slk, s).track_linearize(s["tracks"], s["sigma"], m, chi2=chi2)
    r, H, feat = filt(slk, s2).track_linearize(s2["tracks"], s["sigma"], m, chi2=chi2)
    assert feat[b, :5, 3].tolist() == [0, 0, -1, -1, -2]
    check_linearisation(s2, r, H, feat, chi2, twin)           # (asserts the gate margins and the zero rows)
    keep = np.ones(m, dtype=bool)
    keep[:5 * nr] = False                                     # the other tracks and the other filters: bit for bit
    np.testing.assert_array_equal(r[b, keep], r0[b, keep])
    np.testing.assert_array_equal(H[b, keep], H0[b, keep])
    np.testing.assert_array_equal(feat[b, 5:], feat0[b, 5:])
    for x, y in ((r, r0), (H, H0), (feat, feat0)):
        np.testing.assert_array_equal(np.delete(x, b, axis=0), np.delete(y, b, axis=0))


def test_gate_reads_the_lower_triangle_only(slk):
    # a handle whose strict upper triangle is NaN: any read of it would turn a gamma into NaN and its flag into -2; the
    # twin reads P through tracks_ref.lower().  The scenario of test_flags, so that the gate decides both ways.
    _, s2, b = tr.flag_scenario()
    M, m, N = s2["M"], s2["m"], s2["N"]
    chi2 = tr.CHI2_95[:2 * M - 2]
    Pp = s2["P"].copy()
    Pp[:, np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]] = np.nan
    sp = dict(s2, P=Pp)
    twin = tr.linearize_batch(sp, chi2)
    np.testing.assert_array_equal(twin[2], tr.linearize_batch(s2, chi2)[2])
    assert (twin[2][..., 3] == 1).sum() > 20 and twin[2][b, 4, 3] == -2
    f = slk.Msckf(s2["mean"], Pp)
    for t in (s2["tracks"], dev(s2["tracks"])):
        r, H, feat = f.track_linearize(t, s2["sigma"], m, chi2=chi2)
        if not isinstance(r, np.ndarray):
            r, H, feat = r.cpu().numpy(), H.cpu().numpy(), feat.cpu().numpy()
        check_linearisation(sp, r, H, feat, chi2, twin)


# ------------------------------------------------------------------ 3. bit-exact composition
def composed(slk, f, s, chi2):
    m = s["m"]
    r, H, feat = f.track_linearize(dev(s["tracks"]), s["sigma"], m, chi2=chi2)
    z0, I = dev(np.zeros((s["B"], m))), dev(np.eye(m))
    f.update_ekf(r, z0, H.transpose(1, 2), I, gate=False)
    f.sync()
    return feat.cpu().numpy()


@pytest.mark.parametrize("gated", [False, True], ids=["nochi2", "chi2"])
@pytest.mark.parametrize("shape,lower_only", [(1, False), (4, False), (1, True)], ids=["tile", "general", "tile-lower_only_P"])
def test_update_tracks_is_linearize_plus_update_ekf(slk, shape, lower_only, gated):
    k, M, J, m = tr.SHAPES[shape]
    s = tr.scenario(k, M, J, m)
    chi2 = tr.CHI2_95[:2 * M - 2] if gated else None
    fa, fb, fc = filt(slk, s), filt(slk, s), filt(slk, s)
    if lower_only:
        # three exact-shape UKF steps (k = 8, m = 8: P+ stored as its lower triangle only), no read-out in between; the
        # process input stands still, so that the tracks still belong to the poses
        u0 = np.zeros((s["B"], 13))
        u0[:, 6] = 1.0
        for f in (fa, fb, fc):
            for _ in range(3):
                f.step(slk.PM_DELTA_POSE, u0, s["Q"], s["ukf"]["z"], FEAT, s["ukf"]["feat"], s["ukf"]["R"])
    feat_a = fa.update_tracks(dev(s["tracks"]), s["sigma"], m, chi2=chi2).cpu().numpy()
    feat_b = composed(slk, fb, s, chi2)
    np.testing.assert_array_equal(feat_a, feat_b)
    assert_same_state(fa, fb)
    assert (feat_a[..., 3] == 1).any(axis=1).all(), "a filter without a used track"
    assert (fa.status() == 0).all() and (fa.outliers() == 0).all()
    feat_c = fc.update_tracks(s["tracks"], s["sigma"], m, chi2=chi2)     # the host route gives the same bits
    np.testing.assert_array_equal(feat_a, feat_c)
    assert_same_state(fa, fc)
    assert not np.array_equal(fa.getPk(), s["P"])


@pytest.mark.parametrize("shape,m1,m2", [(1, 60, 120), (0, 24, 48), (0, 48, 24)], ids=["N60-m60-m120", "N24-m24-m48", "N24-m48-m24"])
@pytest.mark.parametrize("gated", [False, True], ids=["nochi2", "chi2"])
def test_update_tracks_between_host_linearisations_of_another_size(slk, shape, m1, m2, gated):
    # update_tracks(m2), a host-route track_linearize(m1) -- it stages its rows in the same workspace of the handle, laid
    # out by m --, update_tracks(m2) again: every update equals the composed route on a handle that never saw the other size
    k, M, J, _ = tr.SHAPES[shape]
    s = dict(tr.scenario(k, M, J, m2), m=m2)
    chi2 = tr.CHI2_95[:2 * M - 2] if gated else None
    fa, fb = filt(slk, s), filt(slk, s)
    lin1 = None
    for _ in range(2):
        feat_a = fa.update_tracks(s["tracks"], s["sigma"], m2, chi2=chi2)
        feat_b = composed(slk, fb, s, chi2)
        np.testing.assert_array_equal(feat_a, feat_b)
        assert_same_state(fa, fb)
        r, H, feat = fa.track_linearize(s["tracks"], s["sigma"], m1, chi2=chi2)
        rd, Hd, featd = fb.track_linearize(dev(s["tracks"]), s["sigma"], m1, chi2=chi2)
        np.testing.assert_array_equal(r, rd.cpu().numpy())
        np.testing.assert_array_equal(H, Hd.cpu().numpy())
        np.testing.assert_array_equal(feat, featd.cpu().numpy())
        assert np.abs(H).max() > 0
    assert not np.array_equal(fa.getPk(), s["P"]) and (fa.status() == 0).all()


# ------------------------------------------------------------------ 4. against the oracle
@pytest.mark.parametrize("k,M,J,m", tr.SHAPES, ids=tr.IDS)
def test_update_tracks_against_oracle(slk, k, M, J, m):
    s = tr.scenario(k, M, J, m)
    t = s["tracks"].copy()
    t[2, :, 1:, 0] = -1.0                                     # filter 2: one slot left per track at the most, nothing used
    s = dict(s, tracks=t)
    chi2 = tr.CHI2_95[:2 * M - 2]
    rt, Ht, ft, _ = tr.linearize_batch(s, chi2)
    f = filt(slk, s)
    feat = f.update_tracks(s["tracks"], s["sigma"], m, chi2=chi2)
    Mg, Pg, st, out = state(f)
    np.testing.assert_array_equal(feat[..., 3], ft[..., 3])
    assert (st == 0).all() and (out == 0).all()
    lay = o.layout(o.MULTI, k)
    worst = [0.0, 0.0]
    for b in range(s["B"]):
        if not (ft[b, :, 3] == 1).any():
            assert b == 2
            assert np.array_equal(Pg[b], s["P"][b]) and np.array_equal(Mg[b], s["mean"][b]), b
            continue
        ref = o.Msckf(k, s["mean"][b], s["P"][b])
        sto, no = ref.update_ekf(rt[b], np.zeros(m), Ht[b], np.eye(m), gate=False)
        assert (sto, no) == (0, 0)
        ep, em = rel(Pg[b], ref.P), float(np.abs(o.boxminus(lay, Mg[b], ref.mean)).max())
        assert ep <= TOL and em <= TOL, (b, ep, em)
        worst = [max(worst[0], ep), max(worst[1], em)]
    assert worst[0] > 0
    print(f"\ntrack update k={k} M={M} J={J} m={m}: worst relative error P {worst[0]:.2e}, mean {worst[1]:.2e}")


# ------------------------------------------------------------------ 5. the step
@pytest.mark.parametrize("route", ["host", "device"])
def test_step_tracks_is_predict_plus_update_tracks(slk, route):
    k, M, J, m = tr.SHAPES[1]
    s = tr.scenario(k, M, J, m)
    chi2 = tr.CHI2_95[:2 * M - 2]
    d = dev if route == "device" else (lambda a: a)
    fa, fb = filt(slk, s), filt(slk, s)
    u, Q, t, c2 = d(s["u"]), d(s["Q"]), d(s["tracks"]), d(chi2)
    sg = d(np.array([s["sigma"]]))
    for _ in range(2):
        feat_a = fa.step_tracks(slk.PM_DELTA_POSE, u, Q, t, sg, m, chi2=c2)
        fb.predict(slk.PM_DELTA_POSE, u, Q)
        fb.sync()
        feat_b = fb.update_tracks(t, sg, m, chi2=c2)
        fa.sync()
        fb.sync()
        if route == "device":
            feat_a, feat_b = feat_a.cpu().numpy(), feat_b.cpu().numpy()
        np.testing.assert_array_equal(feat_a, feat_b)
        assert_same_state(fa, fb)
    assert (fa.status() == 0).all() and not np.array_equal(fa.muState(), s["mean"])


# ------------------------------------------------------------------ 6. refusals and bad indices
def test_refusals_leave_the_filter_untouched(slk):
    k, M, J, m = tr.SHAPES[1]
    s = tr.scenario(k, M, J, m)
    B, N = s["B"], s["N"]
    lib = slk.load_library()
    f = filt(slk, s)
    f.update_tracks(s["tracks"], s["sigma"], m)               # a state that a stray launch would change
    before = state(f)
    t, sg, c2 = np.ascontiguousarray(s["tracks"]), np.array([s["sigma"]]), np.ascontiguousarray(tr.CHI2_95[:2 * M - 2])
    u, Q = np.ascontiguousarray(s["u"]), np.ascontiguousarray(s["Q"])
    r, H, feat = np.empty((B, m)), np.empty((B, N, m)), np.empty((B, J, 4))
    t_bad, t_nan, t_m2 = t.copy(), t.copy(), t.copy()
    t_bad[2, 1, 3, 0] = k + 1
    t_nan[0, 0, 0, 0] = np.nan
    t_m2[1, 2, 4, 0] = -2.0
    sg_b, sg_neg, sg_nan = np.full(B, s["sigma"]), np.array([-0.01]), np.array([np.nan])
    sg_b[3] = 0.0
    good = dict(t=t.ctypes.data, ts=3 * J * M, J=J, M=M, sg=sg.ctypes.data, ss=0, c2=c2.ctypes.data, m=m, r=r.ctypes.data,
                H=H.ctypes.data, feat=feat.ctypes.data, where=slk.HOST, pm=slk.PM_DELTA_POSE, u=u.ctypes.data, us=13,
                Q=Q.ctypes.data, qs=0)
    bad = {
        "null-tracks": dict(t=None), "null-sigma": dict(sg=None), "short-t-stride": dict(ts=3 * J * M - 1),
        "negative-t-stride": dict(ts=-1), "s-stride-2": dict(ss=2), "M-1": dict(M=1), "M-33": dict(M=33), "J-0": dict(J=0),
        "rows-below-N": dict(m=N - 2), "odd-rows": dict(m=m + 1), "rows-above-512": dict(m=514), "rows-below-tracks": dict(J=J + 1, ts=0),
        "unknown-where": dict(where=2), "pose-index-k+1": dict(t=t_bad.ctypes.data), "pose-index-nan": dict(t=t_nan.ctypes.data),
        "pose-index--2": dict(t=t_m2.ctypes.data), "sigma-0": dict(sg=sg_b.ctypes.data, ss=1),
        "sigma-negative": dict(sg=sg_neg.ctypes.data), "sigma-nan": dict(sg=sg_nan.ctypes.data),
    }
    lin_only = {"null-r": dict(r=None), "null-H": dict(H=None)}
    step_only = {"null-u": dict(u=None), "null-Q": dict(Q=None), "short-u-stride": dict(us=12), "short-q-stride": dict(qs=143),
                 "unknown-process-model": dict(pm=99)}

    def call(which, a):
        if which == "linearize":
            return lib.slk_track_linearize(f._h, a["t"], a["ts"], a["J"], a["M"], a["sg"], a["ss"], a["c2"], a["m"], a["r"], a["H"],
                                           a["feat"], a["where"])
        if which == "update":
            return lib.slk_update_tracks(f._h, a["t"], a["ts"], a["J"], a["M"], a["sg"], a["ss"], a["c2"], a["m"], a["feat"], a["where"])
        return lib.slk_step_tracks(f._h, a["pm"], a["u"], a["us"], a["Q"], a["qs"], a["t"], a["ts"], a["J"], a["M"], a["sg"], a["ss"],
                                   a["c2"], a["m"], a["feat"], a["where"])

    for name, kw in list(bad.items()) + list(lin_only.items()) + list(step_only.items()):
        a = dict(good, **kw)
        whichs = ("linearize",) if name in lin_only else (("step",) if name in step_only else ("linearize", "update", "step"))
        for which in whichs:
            assert call(which, a) == slk.E_INVALID, (name, which)
            for x, y in zip(before, state(f)):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} {which}")
    # a Usckf handle
    su = sc.synthetic_usckf(2)
    fu = slk.Usckf(mean=su["mean"], P=su["P"], nfk=3, nfkl=9)
    bu = (fu.muState(), fu.PkAugmentedState(), fu.status())
    tu = np.ascontiguousarray(t[:2])
    mu = 48
    ru, Hu, featu = np.empty((2, mu)), np.empty((2, mu * 48)), np.empty((2, J, 4))
    assert lib.slk_track_linearize(fu._h, tu.ctypes.data, 3 * J * M, 2, M, sg.ctypes.data, 0, None, mu, ru.ctypes.data, Hu.ctypes.data,
                                   featu.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_update_tracks(fu._h, tu.ctypes.data, 3 * J * M, 2, M, sg.ctypes.data, 0, None, mu, featu.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_step_tracks(fu._h, slk.PM_CONST_VELOCITY, su["u"].ctypes.data, 7, Q.ctypes.data, 0, tu.ctypes.data, 3 * J * M, 2, M,
                               sg.ctypes.data, 0, None, mu, featu.ctypes.data, slk.HOST) == slk.E_INVALID
    for x, y in zip(bu, (fu.muState(), fu.PkAugmentedState(), fu.status())):
        np.testing.assert_array_equal(x, y)
    # the unmodified calls are accepted
    for which in ("linearize", "update", "step"):
        assert call(which, good) == 0, which
    assert not np.array_equal(f.muState(), before[0])


@pytest.mark.parametrize("k,M,J,m", [tr.SHAPES[1], tr.SHAPES[4]], ids=["tile", "general"])
@pytest.mark.parametrize("bad", ["k+1", "-2", "nan"])
def test_bad_device_index_skips_that_filter_only(slk, k, M, J, m, bad):
    s = tr.scenario(k, M, J, m)
    tb = s["tracks"].copy()
    tb[1, J - 1, 1, 0] = {"k+1": k + 1, "-2": -2.0, "nan": np.nan}[bad]
    good, f = filt(slk, s), filt(slk, s)
    good.update_tracks(dev(s["tracks"]), s["sigma"], m)
    featf = f.update_tracks(dev(tb), s["sigma"], m).cpu().numpy()
    Mg, Pg, stg, og = state(good)
    Mf, Pf, stf, of = state(f)
    assert stf[1] == slk.ST_BAD_INDEX and of[1] == 0
    assert np.array_equal(Mf[1], s["mean"][1]) and np.array_equal(Pf[1], s["P"][1])
    assert np.isnan(featf[1, :, :3]).all() and (featf[1, :, 3] == 0).all()
    for b in (0, 2, 3):
        assert stf[b] == stg[b] == 0
        assert np.array_equal(Mf[b], Mg[b]) and np.array_equal(Pf[b], Pg[b])
        assert not np.array_equal(Pf[b], s["P"][b])
    # the public linearisation reports the same filter and marks its rows
    f2 = filt(slk, s)
    r, H, feat = f2.track_linearize(dev(tb), s["sigma"], m)
    r, H = r.cpu().numpy(), H.cpu().numpy()
    assert list(f2.status()) == [0, slk.ST_BAD_INDEX, 0, 0]
    assert np.isnan(r[1]).all() and np.isnan(H[1]).all() and not np.isnan(r[[0, 2, 3]]).any() and not np.isnan(H[[0, 2, 3]]).any()
    assert np.array_equal(f2.muState(), s["mean"]) and np.array_equal(f2.getPk(), s["P"])
