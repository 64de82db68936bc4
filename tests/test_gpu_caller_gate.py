"""Caller-side significance tests and the lower-only covariance contract, on every launch route.

The reference's update(z, h, R, mt) takes an arbitrary significance test `mt` (Msckf.hpp:220-277, removeOutliers
:723-754).  Here the test runs on the host, so the update is split into two C calls (include/slk.h): slk_update_innovation
(S and the innovation, an emit-4 launch that leaves the filter alone) and slk_update_selected (the rows the caller kept, a
gate-2 launch reading rowsel [B][m + 2]).  This module checks both against numpy and the fp64 CPU oracle on every Msckf
route of launch_msckf (csrc/slk_api.hip) and on the fused Usckf routes, their host validation, and their equivalence with
the built-in chi-square gate.

The exact-shape updates (Msckf k = 4 .. 8 with m = 8, Usckf N = 48) store only the lower triangle of P+ and leave the
strict upper triangle stale; everything that can run next without a mirror must read the lower triangle only.  Section 5
checks that twice: calls right after such steps against the same calls on a handle whose state went through the host,
and calls on a covariance whose stale region is NaN against a clean twin.

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
rel, mean_err = routes.rel, routes.mean_err
FEAT, POSE, VO = 2, 3, 1          # SLK_MM_FEATURE_PROJ, SLK_MM_POSE_POSITION, SLK_MM_VO_RELATIVE
EXTERNAL = 0


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


# ------------------------------------------------------------------ C ABI helpers (no Python API for the two calls)
def _params(params):
    if params is None:
        return None, 0, None
    a = np.ascontiguousarray(params, dtype=np.float64)
    a = a.reshape(a.shape[0], -1)
    return a.ctypes.data, a.shape[1], a


def _R(R):
    R = np.asarray(R, dtype=np.float64)
    if R.ndim == 2:
        a = np.ascontiguousarray(R.T)
        return a.ctypes.data, 0, a
    a = np.ascontiguousarray(np.transpose(R, (0, 2, 1)))
    return a.ctypes.data, R.shape[1] * R.shape[1], a


def innovation(slk, f, model, params, z, R, Z=None):
    """slk_update_innovation -> (rc, S [B, m, m] row / column indexable, innovation [B, m])."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    B, m = z.shape
    pp, ps, _kp = _params(params)
    rp, rs, _kr = _R(R)
    Zc = None if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
    SI = np.full((B, m * m + m), np.nan)
    rc = slk.load_library().slk_update_innovation(f._h, model, pp, ps, None if Zc is None else Zc.ctypes.data,
                                                  z.ctypes.data, m, rp, rs, SI.ctypes.data, slk.HOST)
    return rc, np.ascontiguousarray(np.transpose(SI[:, :m * m].reshape(B, m, m), (0, 2, 1))), SI[:, m * m:].copy()


def selected(slk, f, model, params, z, R, rowsel, Z=None):
    z = np.ascontiguousarray(z, dtype=np.float64)
    m = z.shape[1]
    pp, ps, _kp = _params(params)
    rp, rs, _kr = _R(R)
    Zc = None if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
    rsel = np.ascontiguousarray(rowsel, dtype=np.int32)
    return slk.load_library().slk_update_selected(f._h, model, pp, ps, None if Zc is None else Zc.ctypes.data,
                                                  z.ctypes.data, m, rp, rs, rsel.ctypes.data, slk.HOST)


def make_rowsel(sels, nouts, m):
    rs = np.zeros((len(sels), m + 2), dtype=np.int32)
    for b, (sel, no) in enumerate(zip(sels, nouts)):
        rs[b, 0], rs[b, 1] = len(sel), no
        rs[b, 2:2 + len(sel)] = sel
    return rs


def select_rows(S, innov, chi2=5.99):
    """The facade's select_rows (include/localization/filters/Msckf.hpp) with mt = accept_mahalanobis_distance: removeOutliers
    (Msckf.hpp:723-754) on S / innovation, the second erase of a rejected block acting on the shifted list (:741-744)."""
    m = len(innov)
    idx = list(range(m))
    cnt, nout, i = m, 0, 0
    while i < cnt // 2:
        p, q = idx[2 * i], idx[2 * i + 1]
        s00, s01, s10, s11 = S[p, p], S[p, q], S[q, p], S[q, q]
        det, r0, r1 = s00 * s11 - s01 * s10, innov[p], innov[q]
        d2 = (r0 * (s11 * r0 - s01 * r1) + r1 * (s00 * r1 - s10 * r0)) / det
        if not d2 < chi2:
            for rep in range(2):
                pos, num = 2 * i + rep, cnt - 1
                if pos < num:
                    idx[pos:num] = idx[pos + 1:num + 1]
                cnt = num
            nout += 1
        else:
            i += 1
    return idx[:cnt], nout


def state(f):
    P = f.getPk() if hasattr(f, "getPk") else f.PkAugmentedState()
    return f.muState(), P


def assert_same_state(a, b, what):
    ma, Pa = state(a)
    mb, Pb = state(b)
    np.testing.assert_array_equal(ma, mb, err_msg=str(what))
    np.testing.assert_array_equal(Pa, Pb, err_msg=str(what))
    np.testing.assert_array_equal(a.status(), b.status(), err_msg=str(what))


# ------------------------------------------------------------------ the Msckf route table
# (k, m, model): the update instantiation a gate-2 call takes (launch_msckf / launch_msckf_n48 / _n60); the emit-4 call
# runs the run-time-m instantiation at the same k.
ROUTES = [(0, 3, POSE),    # <1,64,0,3> closed form
          (0, 4, FEAT),    # <1,64,0>
          (1, 2, FEAT),    # <2,64,1,2>
          (1, 6, FEAT),    # <2,64,1>
          (3, 8, FEAT),    # <2,64>
          (5, 8, FEAT),    # <3,256,5,8> (fast path bails on gate 2)
          (5, 6, FEAT),    # <3,256>
          (7, 6, FEAT),    # <4,256>
          (8, 8, FEAT),    # <4,256,8,8> (fast path bails on gate 2)
          (8, 4, FEAT),    # <4,256,8>
          (8, 32, FEAT),   # <4,256,8>, S factor past the 8 x 8 register path
          (10, 8, FEAT),   # <5,256> + msckf_chol_big_kernel
          (13, 8, FEAT),   # <6,256> + msckf_chol_big_kernel
          (17, 8, FEAT),   # <8,256>
          (22, 8, FEAT),   # <10,512>
          (31, 8, FEAT),   # <13,512,31,8>
          (31, 10, FEAT),  # <13,512>
          (35, 8, FEAT)]   # msckf_update_general_kernel
ROUTE_IDS = [f"k{k}-m{m}-{'pose' if mm == POSE else 'feat'}" for k, m, mm in ROUTES]
# gate 1 and gate 2 take different bodies here: msckf_step_fast against the general body of the same instantiation
FAST_PATHS = {(k, 8) for k in range(4, 9)}


def msckf_case(k, m, model, B, seed):
    """Per-filter inputs of one route: (scenario, params [B, np], z [B, m], numpy model h(b, x))."""
    s = sc.synthetic_msckf(B, k, m=(m if model == FEAT else 2), seed=seed)
    if model == POSE:
        poses = np.array([b % (k + 1) for b in range(B)], dtype=np.float64)
        params = poses[:, None].copy()
        starts = [0 if c == 0 else 13 + 7 * (c - 1) for c in poses.astype(int)]
        rng = np.random.default_rng(seed)
        z = np.stack([s["mean"][b, st:st + 3] for b, st in enumerate(starts)]) + rng.normal(0, 0.05, (B, 3))
        h = lambda b, x: npc.mm_pose_position(x, int(poses[b]))                    # noqa: E731
    else:
        params, z = s["feat"], s["z"]
        h = lambda b, x: npc.mm_feature_proj(x, s["feat"][b])                      # noqa: E731
    return s, np.ascontiguousarray(params), np.ascontiguousarray(z), h


def sigma_Z(f, h):
    X = f.update_sigma_points()
    return X, np.ascontiguousarray([[h(b, x) for x in X[b]] for b in range(X.shape[0])])


def numpy_moments(Z, z, R):
    """meanSigmaPoints / covSigmaPoints + R (Msckf.hpp:234-238, Usckf.hpp:280-282): S [B, m, m], innovation [B, m]."""
    zbar = Z.mean(axis=1)
    D = Z - zbar[:, None, :]
    S = 0.5 * np.einsum("bpi,bpj->bij", D, D) + (R if R.ndim == 3 else R[None])
    return S, z - zbar


def inject_outliers(z, B, m, filters):
    """Gross outliers in some 2-row blocks of some filters (the blocks differ per filter)."""
    z = z.copy()
    for b in filters:
        if b < B:
            for j in range(b % 2, m // 2, 3):
                z[b, 2 * j] += 25.0
    return z


def selections(m):
    """Six per-filter row sets: all; one pair dropped; an odd, non-pair subset; one row; none; every other row (every
    third at m = 32, which keeps 11 rows: more than the 8 x 8 register factor of S)."""
    allr = list(range(m))
    drop = allr[:2] + allr[4:] if m >= 4 else allr[1:]
    odd = [r for r in (0, 3, 5) if r < m]
    wide = allr[::3] if m > 16 else allr[::2]
    return [allr, drop, odd, [m - 1], [], wide]


# ------------------------------------------------------------------ 1. Msckf slk_update_innovation on every route
@pytest.mark.parametrize("k,m,model", ROUTES, ids=ROUTE_IDS)
def test_msckf_innovation_on_every_route(slk, k, m, model):
    """S (the whole m x m matrix), its symmetry and the innovation against numpy on the emitted sigma points; the filter,
    its status and the outlier counts of the previous (gated) update untouched; EXTERNAL Z == the registered model."""
    B = 4
    s, params, z, h = msckf_case(k, m, model, B, seed=0xCA11 + 64 * k + m)
    f = slk.Msckf(s["mean"], s["P"])
    R = s["R"] if model == FEAT else 0.01 * np.eye(3)
    f.update(inject_outliers(z, B, m, (1, 3)), model, params, R, gate=1)      # a previous update with outliers
    out0 = f.outliers()
    assert (f.status() & ~slk.ST_ALL_REJECTED == 0).all()
    f.clear_status()
    if model == FEAT and m >= 4:
        assert out0[1] > 0 and out0[3] > 0, out0
    X, Z = sigma_Z(f, h)
    m0, P0 = state(f)
    rc, S, inn = innovation(slk, f, model, params, z, R)
    assert rc == 0
    assert (f.status() == 0).all()
    np.testing.assert_array_equal(f.outliers(), out0)
    m1, P1 = state(f)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_array_equal(P1, P0)
    Sn, innn = numpy_moments(Z, z, R)
    for b in range(B):
        asym = float(np.abs(S[b] - S[b].T).max() / np.abs(S[b]).max())
        assert asym <= 1e-15, (b, "emitted S not symmetric by", asym)
        assert rel(S[b], Sn[b]) <= 1e-12, (b, rel(S[b], Sn[b]))
        assert np.abs(inn[b] - innn[b]).max() <= 1e-12 * max(1.0, np.abs(z[b]).max()), b
    # EXTERNAL: Z = h(X) computed on the host
    rc, Se, ie = innovation(slk, f, EXTERNAL, None, z, R, Z=Z)
    assert rc == 0 and (f.status() == 0).all()
    assert rel(Se, S) <= 1e-12 and np.abs(ie - inn).max() <= 1e-12
    np.testing.assert_array_equal(state(f)[1], P0)


# ------------------------------------------------------------------ 2. Msckf slk_update_selected on every route
def oracle_selected(k, mean, P, z, h, R, sel):
    """The reference after removeOutliers: the same arithmetic as an ungated update of the model restricted to `sel`."""
    r = o.Msckf(k, mean, P)
    sel = np.asarray(sel, dtype=int)
    st, no = r.update(z[sel], o.mm_python(lambda x: h(x)[sel]), R[np.ix_(sel, sel)], gate=False)
    return st, r


@pytest.mark.parametrize("k,m,model", ROUTES, ids=ROUTE_IDS)
def test_msckf_selected_rows_on_every_route(slk, k, m, model):
    """Six filters of one batch keep different rows (all, one pair dropped, an odd subset, one row, none, every other /
    third row) against the oracle's update of the restricted model; the empty selection leaves its filter bit-identical
    with SLK_ST_ALL_REJECTED; slk_get_outliers returns each filter's rowsel[1]; EXTERNAL Z == the registered model.
    Per-filter dense R on one NT = 3 / 4 route and on the general kernel."""
    B = 6
    s, params, z, h = msckf_case(k, m, model, B, seed=0x5E1 + 64 * k + m)
    lay = o.layout(o.MULTI, k)
    per_filter_R = (k, m) in ((8, 8), (35, 8))
    R = sc.dense_noise(m, B=B, scale=0.01, seed=k + m) if per_filter_R else 0.01 * np.eye(m)
    sels = selections(m)
    nouts = [0, 1, 2, 0, m // 2, 3]
    rsel = make_rowsel(sels, nouts, m)
    f = slk.Msckf(s["mean"], s["P"])
    assert selected(slk, f, model, params, z, R, rsel) == 0
    st = f.status()
    np.testing.assert_array_equal(f.outliers(), nouts)
    M, P = state(f)
    for b, sel in enumerate(sels):
        if not sel:
            assert st[b] == slk.ST_ALL_REJECTED, (b, st[b])
            np.testing.assert_array_equal(M[b], s["mean"][b])
            np.testing.assert_array_equal(P[b], s["P"][b])
            continue
        assert st[b] == 0, (b, sel, st[b])
        Rb = R[b] if per_filter_R else R
        stc, r = oracle_selected(k, s["mean"][b], s["P"][b], z[b], lambda x, b=b: h(b, x), Rb, sel)
        assert stc == 0
        assert rel(P[b], r.P) <= TOL, (b, sel, rel(P[b], r.P))
        assert mean_err(lay, M[b], r.mean) <= TOL, (b, sel)
    # EXTERNAL Z on a twin
    g = slk.Msckf(s["mean"], s["P"])
    _, Z = sigma_Z(g, h)
    assert selected(slk, g, EXTERNAL, None, z, R, rsel, Z=Z) == 0
    np.testing.assert_array_equal(g.status(), st)
    np.testing.assert_array_equal(g.outliers(), nouts)
    Mg, Pg = state(g)
    for b in range(B):
        assert rel(Pg[b], P[b]) <= TOL and mean_err(lay, Mg[b], M[b]) <= TOL, b


@pytest.mark.parametrize("k,m,model", ROUTES, ids=ROUTE_IDS)
def test_msckf_selected_equals_built_in_gate(slk, k, m, model):
    """select_rows with chi2_0.95(2) = 5.99 on slk_update_innovation's output, then slk_update_selected == slk_update with
    gate 1 on a twin handle, with gross outliers in some blocks of some filters: the same outlier counts and status, and a
    bit-identical state wherever both calls run the same body (<= 1e-12 on the exact-shape fast paths, whose operation
    order differs)."""
    B = 6
    s, params, z, h = msckf_case(k, m, model, B, seed=0x6A7E + 64 * k + m)
    z = inject_outliers(z, B, m, (1, 3, 4)) if model == FEAT else z
    if model == POSE:
        z = z.copy()
        z[1, 0] += 5.0
        z[4, 1] -= 5.0
    R = s["R"] if model == FEAT else 0.01 * np.eye(3)
    f = slk.Msckf(s["mean"], s["P"])
    g = slk.Msckf(s["mean"], s["P"])
    rc, S, inn = innovation(slk, f, model, params, z, R)
    assert rc == 0
    picks = [select_rows(S[b], inn[b]) for b in range(B)]
    rsel = make_rowsel([p[0] for p in picks], [p[1] for p in picks], m)
    assert selected(slk, f, model, params, z, R, rsel) == 0
    g.update(z, model, params, R, gate=1)
    np.testing.assert_array_equal(f.outliers(), g.outliers())
    np.testing.assert_array_equal(f.status(), g.status())
    np.testing.assert_array_equal(f.outliers(), [p[1] for p in picks])
    if model == FEAT and m >= 4:
        assert (f.outliers()[[1, 3]] > 0).all()
    Mf, Pf = state(f)
    Mg, Pg = state(g)
    if (k, m) in FAST_PATHS:
        lay = o.layout(o.MULTI, k)
        for b in range(B):
            assert rel(Pf[b], Pg[b]) <= 1e-12 and mean_err(lay, Mf[b], Mg[b]) <= 1e-12, b
    else:
        np.testing.assert_array_equal(Mf, Mg)
        np.testing.assert_array_equal(Pf, Pg)


@pytest.mark.parametrize("k,m,model", [(0, 3, POSE), (8, 8, FEAT), (8, 32, FEAT), (35, 8, FEAT)],
                         ids=["k0-m3-pose", "k8-m8", "k8-m32", "k35-m8-general"])
def test_msckf_selected_device_resident(slk, k, m, model):
    """where = SLK_DEVICE: z, per-filter R, per-filter parameters and rowsel (int32) as torch device tensors == the host
    call on a twin, bit for bit."""
    import torch
    B = 6
    s, params, z, h = msckf_case(k, m, model, B, seed=0xDE7 + k + m)
    R = sc.dense_noise(m, B=B, scale=0.01, seed=3 * k + m)
    rsel = make_rowsel(selections(m), [1, 0, 2, 3, 4, 5], m)
    f = slk.Msckf(s["mean"], s["P"])
    assert selected(slk, f, model, params, z, R, rsel) == 0
    g = slk.Msckf(s["mean"], s["P"])
    dev = torch.device("cuda", 0)
    pp = torch.from_numpy(np.ascontiguousarray(params.reshape(B, -1))).to(dev)
    zz = torch.from_numpy(z).to(dev)
    RR = torch.from_numpy(np.ascontiguousarray(np.transpose(R, (0, 2, 1)))).to(dev)
    rr = torch.from_numpy(rsel).to(dev)
    assert rr.dtype == torch.int32
    torch.cuda.synchronize()                           # (the handle's stream does not wait for torch's)
    rc = slk.load_library().slk_update_selected(g._h, model, pp.data_ptr(), pp.shape[1], None, zz.data_ptr(), m,
                                                RR.data_ptr(), m * m, rr.data_ptr(), slk.DEVICE)
    assert rc == 0
    g.sync()
    assert_same_state(f, g, "device-resident")
    np.testing.assert_array_equal(f.outliers(), g.outliers())


def test_msckf_selected_full_batch(slk):
    """k = 8, m = 8, B = 4097 with a random selection per filter (0 .. 8 rows): statuses, outlier counts, the rejected
    filters bit-identical, batch properties of all, 64 sampled filters against the oracle."""
    B, k, m = 4097, 8, 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0xB4097)
    lay = o.layout(o.MULTI, k)
    rng = np.random.default_rng(4097)
    sels = [sorted(rng.choice(m, size=int(rng.integers(0, m + 1)), replace=False).tolist()) for _ in range(B)]
    nouts = rng.integers(0, 5, B)
    rsel = make_rowsel(sels, nouts, m)
    f = slk.Msckf(s["mean"], s["P"])
    assert selected(slk, f, FEAT, s["feat"], s["z"], s["R"], rsel) == 0
    st = f.status()
    empty = np.array([len(x) == 0 for x in sels])
    assert empty.any() and (~empty).any()
    np.testing.assert_array_equal(st, np.where(empty, slk.ST_ALL_REJECTED, 0))
    np.testing.assert_array_equal(f.outliers(), nouts)
    M, P = state(f)
    np.testing.assert_array_equal(M[empty], s["mean"][empty])
    np.testing.assert_array_equal(P[empty], s["P"][empty])
    routes.check_batch_properties(P, M, [3] + [13 + 7 * c + 3 for c in range(k)])
    for b in routes.sample_idx(B, 4097):
        if not sels[b]:
            continue
        stc, r = oracle_selected(k, s["mean"][b], s["P"][b], s["z"][b], lambda x, b=b: npc.mm_feature_proj(x, s["feat"][b]),
                                 s["R"], sels[b])
        assert stc == 0
        assert rel(P[b], r.P) <= TOL and mean_err(lay, M[b], r.mean) <= TOL, (b, sels[b])


# ------------------------------------------------------------------ 3. host-side rejection
def test_host_side_rejection(slk):
    """slk_update_selected / slk_update_innovation return SLK_E_INVALID before any launch, the filter bit-identical."""
    B, k, m = 2, 8, 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0xBAD)
    f = slk.Msckf(s["mean"], s["P"])
    m0, P0 = state(f)
    good = make_rowsel([[0, 1, 2], [4, 5]], [0, 1], m)
    assert selected(slk, f, FEAT, s["feat"], s["z"], s["R"], good) == 0      # (the template of the bad tables is valid)
    f = slk.Msckf(s["mean"], s["P"])

    def bad(edit):
        r = good.copy()
        edit(r)
        return r
    tables = {"rowsel[0] < 0": bad(lambda r: r.__setitem__((1, 0), -1)),
              "rowsel[0] > m": bad(lambda r: r.__setitem__((1, 0), m + 1)),
              "rowsel[1] < 0": bad(lambda r: r.__setitem__((0, 1), -1)),
              "row index < 0": bad(lambda r: r.__setitem__((1, 3), -1)),
              "row index >= m": bad(lambda r: r.__setitem__((0, 4), m))}
    for what, t in tables.items():
        assert selected(slk, f, FEAT, s["feat"], s["z"], s["R"], t) == slk.E_INVALID, what
    X = f.update_sigma_points()
    Z = np.ascontiguousarray([[npc.mm_feature_proj(x, s["feat"][b]) for x in X[b]] for b in range(B)])
    assert selected(slk, f, EXTERNAL, None, s["z"], s["R"], good) == slk.E_INVALID            # EXTERNAL without Z
    assert selected(slk, f, FEAT, s["feat"], s["z"], s["R"], good, Z=Z) == slk.E_INVALID      # registered model with Z
    rc, _, _ = innovation(slk, f, EXTERNAL, None, s["z"], s["R"])
    assert rc == slk.E_INVALID
    rc, _, _ = innovation(slk, f, FEAT, s["feat"], s["z"], s["R"], Z=Z)
    assert rc == slk.E_INVALID
    # m = 33 rows on Msckf
    m33 = 33
    Z33 = np.zeros((B, X.shape[1], m33))
    assert selected(slk, f, EXTERNAL, None, np.zeros((B, m33)), 0.01 * np.eye(m33), make_rowsel([[0], [1]], [0, 0], m33),
                    Z=Z33) == slk.E_INVALID
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    m1, P1 = state(f)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_array_equal(P1, P0)
    # a Usckf handle
    u = sc.synthetic_usckf(B)
    g = slk.Usckf(mean=u["mean"], P=u["P"], nfk=3, nfkl=9)
    feat, zf = sc.usckf_features(u["mean"], poses=(0, 1, 2, 0))
    assert selected(slk, g, FEAT, feat, zf, 0.01 * np.eye(8), good) == slk.E_INVALID
    np.testing.assert_array_equal(g.muState(), u["mean"])
    np.testing.assert_array_equal(g.PkAugmentedState(), u["P"])
    assert (g.status() == 0).all()


# ------------------------------------------------------------------ 4. Usckf slk_update_innovation on the fused routes
USCKF_SHAPES = [(3, 9), (3, 18), (6, 30), (6, 54)]      # N = 48 (usckf_kernel<3>), 57, 72, 96 (usckf_kernel<4..6>)


def usckf_case(s, model, nfk):
    B = s["B"]
    if model == VO:
        return None, s["z"], s["R"], lambda b, x: npc.mm_vo_relative(x, nfk)
    if model == FEAT:
        feat, z = sc.usckf_features(s["mean"], poses=(0, 2), seed=nfk)
        return feat, z, 0.01 * np.eye(4), lambda b, x: npc.mm_feature_proj(x, feat[b], kind="aug")
    poses = np.array([b % 3 for b in range(B)], dtype=np.float64)
    z = np.stack([s["mean"][b, 13 * int(c):13 * int(c) + 3] for b, c in enumerate(poses)]) + 0.03
    return poses[:, None].copy(), z, 0.01 * np.eye(3), lambda b, x: npc.mm_pose_position(x, int(poses[b]), kind="aug")


@pytest.mark.parametrize("model", [VO, FEAT, POSE], ids=["vo", "feat", "pose"])
@pytest.mark.parametrize("nfk,nfkl", USCKF_SHAPES, ids=[f"N{36 + a + b}" for a, b in USCKF_SHAPES])
def test_usckf_innovation_on_fused_routes(slk, nfk, nfkl, model):
    """S (whole matrix) and the innovation == numpy on the emitted sigma points, the filter untouched, EXTERNAL Z == the
    registered model."""
    B = 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x1E40 + nfk + nfkl)
    params, z, R, h = usckf_case(s, model, nfk)
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    X, Z = sigma_Z(f, h)
    rc, S, inn = innovation(slk, f, model, params, z, R)
    assert rc == 0 and (f.status() == 0).all()
    np.testing.assert_array_equal(f.muState(), s["mean"])
    np.testing.assert_array_equal(f.PkAugmentedState(), s["P"])
    Sn, innn = numpy_moments(Z, z, R)
    for b in range(B):
        asym = float(np.abs(S[b] - S[b].T).max() / np.abs(S[b]).max())
        assert asym <= 1e-15, (b, "emitted S not symmetric by", asym)
        assert rel(S[b], Sn[b]) <= 1e-12, (b, rel(S[b], Sn[b]))
        assert np.abs(inn[b] - innn[b]).max() <= 1e-12 * max(1.0, np.abs(z[b]).max()), b
    rc, Se, ie = innovation(slk, f, EXTERNAL, None, z, R, Z=Z)
    assert rc == 0 and (f.status() == 0).all()
    assert rel(Se, S) <= 1e-12 and np.abs(ie - inn).max() <= 1e-12


def test_usckf_innovation_interleaved_with_unit_shape_steps(slk):
    """N = 48: step, innovation, step, innovation, step == three plain steps (bit-identical mean and P), and each
    interleaved innovation == the same call on a handle that received the state through the host.  The emit-4 launch
    mirrors the stale upper triangle first; that must change nothing a later step reads."""
    B = 4
    s = sc.synthetic_usckf(B, seed=0x1E48)

    def new(mean=None, P=None):
        return slk.Usckf(mean=s["mean"] if mean is None else mean, P=s["P"] if P is None else P, nfk=3, nfkl=9)

    def step(f):
        f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])

    a = new()
    got = []
    for i in range(3):
        step(a)
        if i < 2:
            rc, S, inn = innovation(slk, a, VO, None, s["z"], s["R"])
            assert rc == 0
            got.append((S, inn))
    plain = new()
    for _ in range(3):
        step(plain)
    assert (a.status() == 0).all()
    assert_same_state(a, plain, "interleaved steps")
    for n, (S, inn) in enumerate(got, start=1):
        c = new()
        for _ in range(n):
            step(c)
        hst = new(c.muState(), c.PkAugmentedState())
        rc, Sh, ih = innovation(slk, hst, VO, None, s["z"], s["R"])
        assert rc == 0
        np.testing.assert_array_equal(S, Sh, err_msg=f"S after {n} steps")
        np.testing.assert_array_equal(inn, ih, err_msg=f"innovation after {n} steps")


# ------------------------------------------------------------------ 5a. calls right after lower-only steps
def msckf_calls(slk, s, k, B):
    """Every call that may follow an exact-shape step without a read-out: name -> fn(filter) -> extra outputs."""
    N = s["N"]
    pose = np.array([[float(b % (k + 1))] for b in range(B)])
    zpose = s["mean"][:, 0:3] + 0.04
    e = sc.synthetic_ekf(B, k, N + 8, seed=0xEC0 + k, outliers=False)       # (every row kept: the update is applied)
    rsel = make_rowsel([[0, 1, 4, 5], [2, 3, 6], [7], [0, 1, 2, 3, 4, 5, 6, 7]][:B], [2, 1, 3, 0][:B], 8)

    def precision(mode):
        def run(f):
            f.set_rebuild_precision(mode)
            f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"], gate=1)
        return run

    def ekf(f):
        f.update_ekf(e["z"], e["zmean"], e["H"], e["R"], gate=False)
        return f.outliers()

    def innov(f):
        rc, S, inn = innovation(slk, f, FEAT, s["feat"], s["z"], s["R"])
        assert rc == 0
        return S, inn

    return {
        "selected": lambda f: selected(slk, f, FEAT, s["feat"], s["z"], s["R"], rsel),
        "innovation": innov,
        "m4": lambda f: f.update(s["z"][:, :4], slk.MM_FEATURE_PROJ, s["feat"][:, :2], 0.01 * np.eye(4), gate=1),
        "pose_position": lambda f: f.update(zpose, slk.MM_POSE_POSITION, pose, 0.01 * np.eye(3), gate=0),
        "ekf": ekf,
        "predict": lambda f: f.predict(slk.PM_DELTA_POSE, s["u"], s["Q"]),
        "rebuild_f32": precision(1),
        "rebuild_bf16": precision(2),
    }


@pytest.mark.parametrize("k", [5, 8])
def test_msckf_calls_after_lower_only_steps(slk, k):
    """Three exact-shape steps (m = 8, FEATURE_PROJ) with no read-out, then each call on its own handle == the same call on
    a twin whose state went through the host (set_state(muState(), getPk())): bit-identical mean, P, status, outputs."""
    B = 4
    s = sc.synthetic_msckf(B, k, m=8, seed=0x10E0 + k)

    def stepped():
        f = slk.Msckf(s["mean"], s["P"])
        for _ in range(3):
            f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
        return f

    ref = stepped()
    M0, P0 = state(ref)
    assert (ref.status() == 0).all()
    for name, call in msckf_calls(slk, s, k, B).items():
        a = stepped()
        b = slk.Msckf(M0, P0)
        ra, rb = call(a), call(b)
        if isinstance(ra, tuple):
            for x, y in zip(ra, rb):
                np.testing.assert_array_equal(x, y, err_msg=name)
        elif ra is not None:
            np.testing.assert_array_equal(ra, rb, err_msg=name)
        assert_same_state(a, b, name)
        assert (a.status() & ~slk.ST_ALL_REJECTED == 0).all(), (name, a.status())      # (the call was applied)
        np.testing.assert_array_equal(a.outliers(), b.outliers(), err_msg=name)


def usckf_calls(slk, s, B):
    lay = o.layout(o.AUGMENTED, 0, 3, 9)
    truth = np.stack([o.boxplus(lay, s["mean"][b], np.random.default_rng(b).normal(0, 0.05, s["N"])) for b in range(B)])
    noise = np.random.default_rng(48).normal(0, 1, (B, 3, s["N"]))
    feat, zw = sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(17)), seed=34)
    return {
        "exact_update": lambda f: f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"], gate=0),
        "wide_update": lambda f: f.update(zw, slk.MM_FEATURE_PROJ, feat, 0.01 * np.eye(34), gate=0),
        "nees": lambda f: f.nees(truth),
        "sample_states": lambda f: f.sample_states(noise),
    }


@pytest.mark.parametrize("then_predict", [False, True], ids=["after-steps", "after-predict"])
def test_usckf_calls_after_lower_only_steps(slk, then_predict):
    """Unit shape (N = 48): three lower-only steps (and a predict-only call), then the exact update, a wide update (m = 34),
    nees and sample_states == the same calls on a twin whose state went through the host, bit for bit."""
    B = 4
    s = sc.synthetic_usckf(B, seed=0x1E4A)

    def stepped():
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
        for _ in range(3):
            f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
        if then_predict:
            f.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"])
        return f

    ref = stepped()
    M0, P0 = state(ref)
    assert (ref.status() == 0).all()
    for name, call in usckf_calls(slk, s, B).items():
        a = stepped()
        b = slk.Usckf(mean=M0, P=P0, nfk=3, nfkl=9)
        ra, rb = call(a), call(b)
        if ra is not None:
            np.testing.assert_array_equal(ra, rb, err_msg=name)
        assert_same_state(a, b, name)


# ------------------------------------------------------------------ 5b. a poisoned stale region
def poisoned(P, region):
    Pn = P.copy()
    Pn[:, region[0], region[1]] = np.nan
    return Pn


def compare_poisoned(clean, pois, what):
    assert (clean.status() & (o.LLT_FAIL | o.SINGULAR) == 0).all(), (what, clean.status())       # (LLT_FAIL, SINGULAR: applied)
    np.testing.assert_array_equal(pois.status(), clean.status(), err_msg=str(what))
    Mc, Pc = state(clean)
    Mp, Pp = state(pois)
    np.testing.assert_array_equal(Mp, Mc, err_msg=str(what))
    il = np.tril_indices(Pc.shape[1])
    np.testing.assert_array_equal(Pp[:, il[0], il[1]], Pc[:, il[0], il[1]], err_msg=str(what))


@pytest.mark.parametrize("k", [4, 5, 6, 7, 8])
def test_msckf_poisoned_upper_triangle(slk, k):
    """The strict upper triangle outside the 16 x 16 diagonal tiles -- what the fast path leaves stale -- is NaN
    (set_state: upper_stale false, so nothing mirrors it): every emit-0 call that can follow a fast step gives the clean
    twin's status, mean and lower triangle."""
    B, m = 3, 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0xBAAD + k)
    N = s["N"]
    i, j = np.triu_indices(N, 1)
    keep = i // 16 != j // 16
    Pn = poisoned(s["P"], (i[keep], j[keep]))
    pose = np.array([[float(b % (k + 1))] for b in range(B)])
    zpose = s["mean"][:, 0:3] + 0.04
    zo = inject_outliers(s["z"], B, m, (1,))
    rsel = make_rowsel([[0, 1, 2, 3, 4, 5, 6, 7], [0, 3, 5], [6, 7]], [0, 2, 3], m)

    def step(gate, prec=0):
        def run(f):
            if prec:
                f.set_rebuild_precision(prec)
            f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], zo, slk.MM_FEATURE_PROJ, s["feat"], s["R"], gate=gate)
        return run

    calls = {
        "predict": lambda f: f.predict(slk.PM_DELTA_POSE, s["u"], s["Q"]),
        "step_gate0": step(0), "step_gate1": step(1),
        "update_gate0": lambda f: f.update(zo, slk.MM_FEATURE_PROJ, s["feat"], s["R"], gate=0),
        "update_gate1": lambda f: f.update(zo, slk.MM_FEATURE_PROJ, s["feat"], s["R"], gate=1),
        "update_gate2": lambda f: selected(slk, f, FEAT, s["feat"], zo, s["R"], rsel),
        "update_m4": lambda f: f.update(s["z"][:, :4], slk.MM_FEATURE_PROJ, s["feat"][:, :2], 0.01 * np.eye(4), gate=1),
        "step_m4": lambda f: f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"][:, :4], slk.MM_FEATURE_PROJ, s["feat"][:, :2],
                                    0.01 * np.eye(4), gate=1),
        "pose_position": lambda f: f.update(zpose, slk.MM_POSE_POSITION, pose, 0.01 * np.eye(3), gate=0),
        "rebuild_f32": step(1, 1), "rebuild_bf16": step(1, 2),
    }
    for name, call in calls.items():
        clean = slk.Msckf(s["mean"], s["P"])
        pois = slk.Msckf(s["mean"], Pn)
        assert call(clean) in (None, 0) and call(pois) in (None, 0)
        compare_poisoned(clean, pois, (k, name))


def test_usckf_poisoned_upper_triangle(slk):
    """Unit shape (N = 48): the whole strict upper triangle NaN (its predict keeps only the lower triangle proper):
    predict, the exact update, the step and a wide update (m = 34) give the clean twin's status, mean and lower
    triangle."""
    B = 3
    s = sc.synthetic_usckf(B, seed=0xBAAE)
    Pn = poisoned(s["P"], np.triu_indices(s["N"], 1))
    feat, zw = sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(17)), seed=35)
    calls = {
        "predict": lambda f: f.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"]),
        "exact_update": lambda f: f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"], gate=0),
        "step": lambda f: f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"]),
        "wide_update": lambda f: f.update(zw, slk.MM_FEATURE_PROJ, feat, 0.01 * np.eye(34), gate=0),
    }
    for name, call in calls.items():
        clean = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
        pois = slk.Usckf(mean=s["mean"], P=Pn, nfk=3, nfkl=9)
        call(clean)
        call(pois)
        compare_poisoned(clean, pois, name)
