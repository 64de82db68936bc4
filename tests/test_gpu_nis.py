"""Innovation consistency (slk_nis) and standard deviations (slk_get_sigma) against numpy.

Reference for every number: numpy on the CPU.  S and the innovation come from the sigma points the library emits
(slk_update_sigma_points), mapped through the numpy measurement models of oracle/np_check.py and folded by numpy_moments
exactly as tests/test_gpu_caller_gate.py::test_msckf_innovation_on_every_route builds them; then
nis = nu @ solve(S, nu), logdet = slogdet(S)[1], sigma = sqrt(diag(P)).

Tolerances: rtol 1e-9 on nis, atol 1e-9 * m on logdet -- the project's own NEES figures (test_gpu_consistency.py: the
same quadratic form through the same factorisation).  They hold for a well-conditioned S only, so every compared case
asserts cond(S_ref) <= 1e4 on the CPU first (a condition on the inputs: with m <= 128 it bounds the solve error by about
cond * m * eps ~ 1e-10); no case is skipped for failing it.

Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import np_check as npc
import scenarios as sc
from nis_support import (assert_stats, innovation, nis_c, nis_device, numpy_moments, reference, sigma_Z,  # noqa: F401
                         state)

pytestmark = pytest.mark.gpu
FEAT, POSE, VO, EXTERNAL = 2, 3, 1, 0          # SLK_MM_FEATURE_PROJ, SLK_MM_POSE_POSITION, SLK_MM_VO_RELATIVE, SLK_MODEL_EXTERNAL


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


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


# the ROUTES of test_gpu_caller_gate.py (the fast path, the one-wave, large and global-workspace kernels), then m = 20 and
# m = 32 at k = 8 and the position fix at k = 8; every case also runs as SLK_MODEL_EXTERNAL with Z = h(X) from the host
ROUTES = [(0, 3, POSE), (0, 4, FEAT), (1, 2, FEAT), (1, 6, FEAT), (3, 8, FEAT), (5, 8, FEAT), (5, 6, FEAT), (7, 6, FEAT),
          (8, 8, FEAT), (8, 4, FEAT), (8, 32, FEAT), (10, 8, FEAT), (13, 8, FEAT), (17, 8, FEAT), (22, 8, FEAT), (31, 8, FEAT),
          (31, 10, FEAT), (35, 8, FEAT),
          (8, 20, FEAT), (8, 3, POSE)]
ROUTE_IDS = [f"k{k}-m{m}-{'pose' if mm == POSE else 'feat'}" for k, m, mm in ROUTES]


def run_every_layout(slk, f, model, params, z, h, m, what):
    """shared R and per-filter dense R on the host route, EXTERNAL Z, and the device route, each against numpy"""
    B = z.shape[0]
    X, Z = sigma_Z(f, h)
    m0, P0 = state(f)
    for name, R in (("shared", 0.01 * np.eye(m)), ("per-filter", sc.dense_noise(m, B=B, scale=0.01, seed=m + B))):
        Sn, nun = numpy_moments(Z, z, R)
        want_n, want_ld = reference(Sn, nun, (what, name))
        rc, n, ld = nis_c(slk, f, model, params, z, R)
        assert rc == 0
        assert_stats(n, ld, want_n, want_ld, m, (what, name, "host"))
        rc, ne, lde = nis_c(slk, f, EXTERNAL, None, z, R, Z=Z)
        assert rc == 0
        assert_stats(ne, lde, want_n, want_ld, m, (what, name, "external"))
        nd, ldd = nis_device(slk, f, model, params, z, R)
        assert_stats(nd, ldd, want_n, want_ld, m, (what, name, "device"))
        np.testing.assert_array_equal(nd, n)              # (the same launches on the same data)
        np.testing.assert_array_equal(ldd, ld)
        rc, n1, ld1 = nis_c(slk, f, model, params, z, R, want_logdet=False)
        assert rc == 0 and (ld1 == -7.0).all()
        np.testing.assert_array_equal(n1, n)
    assert (f.status() == 0).all()
    m1, P1 = state(f)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_array_equal(P1, P0)


# ------------------------------------------------------------------ 1. slk_nis on every route
@pytest.mark.parametrize("k,m,model", ROUTES, ids=ROUTE_IDS)
def test_msckf_nis_on_every_route(slk, k, m, model):
    B = 4
    s, params, z, h = msckf_case(k, m, model, B, seed=0x215 + 64 * k + m)
    f = slk.Msckf(s["mean"], s["P"])
    run_every_layout(slk, f, model, params, z, h, m, ("msckf", k, m))


def usckf_feat(s, nfeat, seed):
    feat, z = sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(nfeat)), seed=seed)
    return feat, z, (lambda b, x: npc.mm_feature_proj(x, feat[b], kind="aug"))


USCKF = [("unit-N48-m3-vo", 3, 9, VO, 3), ("fused-N72-m4-feat", 6, 30, FEAT, 4), ("fused-N96-m3-pose", 6, 54, POSE, 3),
         ("large-N132-m8-feat", 36, 60, FEAT, 8), ("large-N108-m36-vo", 36, 36, VO, 36),
         ("wide-N48-m34", 3, 9, FEAT, 34), ("wide-N96-m64", 12, 48, FEAT, 64), ("wide-N164-m128", 30, 98, FEAT, 128)]


@pytest.mark.parametrize("name,nfk,nfkl,model,m", USCKF, ids=[u[0] for u in USCKF])
def test_usckf_nis_on_every_route(slk, name, nfk, nfkl, model, m):
    B = 3
    s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl, seed=0x215 + nfk + nfkl)
    if model == VO:
        params, z, h = None, s["z"], (lambda b, x: npc.mm_vo_relative(x, nfk))
    elif model == FEAT:
        params, z, h = usckf_feat(s, m // 2, seed=nfk)
    else:
        poses = np.array([b % 3 for b in range(B)], dtype=np.float64)
        z = np.stack([s["mean"][b, 13 * int(c):13 * int(c) + 3] for b, c in enumerate(poses)]) + 0.03
        params, h = poses[:, None].copy(), (lambda b, x: npc.mm_pose_position(x, int(poses[b]), kind="aug"))
    f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
    run_every_layout(slk, f, model, params, np.ascontiguousarray(z), h, m, name)


# ------------------------------------------------------------------ 2. equality with the existing emission, read-only
def innovation_device(slk, f, model, params, z, R):
    """slk_update_innovation with where = SLK_DEVICE (torch tensors in, SI written to device memory) ->
    (S [B, m, m] row / column indexable, innovation [B, m])."""
    import torch
    dev = torch.device("cuda", 0)
    B, m = z.shape
    R = np.asarray(R, dtype=np.float64)
    Rd = torch.from_numpy(np.ascontiguousarray(R.T if R.ndim == 2 else np.transpose(R, (0, 2, 1)))).to(dev)
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    pd = None if params is None else torch.from_numpy(np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(B, -1))).to(dev)
    SI = torch.full((B, m * m + m), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()                           # (the handle's stream does not wait for torch's)
    rc = slk.load_library().slk_update_innovation(f._h, model, None if pd is None else pd.data_ptr(),
                                                  0 if pd is None else pd.shape[1], None, zd.data_ptr(), m, Rd.data_ptr(),
                                                  0 if R.ndim == 2 else m * m, SI.data_ptr(), slk.DEVICE)
    assert rc == 0
    f.sync()
    SI = SI.cpu().numpy()
    return np.ascontiguousarray(np.transpose(SI[:, :m * m].reshape(B, m, m), (0, 2, 1))), SI[:, m * m:].copy()


class RawCov:
    """The handle's covariance buffer as it sits in device memory (column-major: element (i, j) at [b, j, i]), read
    through the HIP runtime at an address fetched while P was complete -- fetching it later would complete P.  Steps and
    updates keep the buffer (only window operations and setMeasurement move the state)."""

    def __init__(self, f):
        import ctypes as C
        self.C, self.rt = C, C.CDLL("libamdhip64.so")
        self.f, self.B, self.N = f, f.B, f.N
        _, self.ptr = f.device_pointers()
        i, j = np.triu_indices(self.N, 1)
        keep = i // 16 != j // 16                      # what the lower-only kernels leave stale: outside the diagonal tiles
        self.i, self.j = i[keep], j[keep]

    def upper(self):
        C = self.C
        self.f.sync()
        host = np.empty((self.B, self.N, self.N))
        assert self.rt.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(self.ptr), C.c_size_t(host.nbytes), 2) == 0
        return host[:, self.j, self.i]                 # P(i, j), i < j


def check_read_only_on_a_lower_only_P(slk, prepared, call_nis, emitted, m, what, expect_stale):
    """prepared() -> a filter after its steps / previous update, nothing read out of it.  slk_nis runs on one such filter
    while its P is still lower-only (only status() and outliers(), which complete nothing, are read before), a twin
    that ran the same calls WITHOUT slk_nis is the reference state.  The raw covariance buffer shows what happened: its
    strict upper triangle is stale before the call and complete after it (slk_nis, like slk_update_innovation,
    completes a lower-only P first), and the completed matrix is the twin's."""
    f, raw = prepared()
    twin, _ = prepared()
    st0, out0 = f.status(), f.outliers()
    before = raw.upper()
    rc, n, ld = call_nis(f)                            # P is lower-only here where expect_stale
    assert rc == 0
    after = raw.upper()
    np.testing.assert_array_equal(f.status(), st0, err_msg=str(what))
    np.testing.assert_array_equal(f.outliers(), out0, err_msg=str(what))
    mt, Pt = state(twin)
    want_upper = Pt[:, raw.i, raw.j]
    if expect_stale:
        assert not np.array_equal(before, want_upper), (what, "P was not lower-only at the call")
        np.testing.assert_array_equal(after, want_upper, err_msg=str(what))
    else:
        np.testing.assert_array_equal(before, want_upper, err_msg=str(what))
        np.testing.assert_array_equal(after, before, err_msg=str(what))
    mf, Pf = state(f)
    np.testing.assert_array_equal(mf, mt, err_msg=str(what))
    np.testing.assert_array_equal(Pf, Pt, err_msg=str(what))
    np.testing.assert_array_equal(f.status(), twin.status(), err_msg=str(what))
    np.testing.assert_array_equal(f.outliers(), twin.outliers(), err_msg=str(what))
    S, inn = emitted(f)                                # slk_update_innovation, SLK_DEVICE, same handle
    want_n, want_ld = reference(S, inn, what)
    assert_stats(n, ld, want_n, want_ld, m, what)
    return n, ld, (mt, Pt)


@pytest.mark.parametrize("k,m", [(8, 8), (8, 32), (5, 8), (1, 6)])
def test_nis_equals_numpy_on_the_emitted_innovation(slk, k, m):
    """slk_nis against numpy on the SI slk_update_innovation (SLK_DEVICE) returns for the same handle; mean, P, status and
    the outlier counts of a previous gated update untouched -- also when P is lower-only at the call: after three
    fast-path steps and / or the exact-shape gated update (m = 8 at k = 5, 8), with nothing read out in between."""
    B = 4
    s, params, z, h = msckf_case(k, m, FEAT, B, seed=0xE41 + k + m)
    R = 0.01 * np.eye(m)
    zo = z.copy()
    zo[1, 0] += 25.0
    zo[3, 1] += 25.0
    for steps in ((0, 3) if m == 8 else (0,)):                         # (the exact-shape steps are those of m = 8)
        def prepared():
            f = slk.Msckf(s["mean"], s["P"])
            raw = RawCov(f)
            for _ in range(steps):
                f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
            f.update(zo, FEAT, params, R, gate=1)                      # a previous update with outliers
            return f, raw
        n, ld, (mt, Pt) = check_read_only_on_a_lower_only_P(
            slk, prepared, lambda f: nis_c(slk, f, FEAT, params, z, R), lambda f: innovation_device(slk, f, FEAT, params, z, R),
            m, ("emitted", k, m, steps), expect_stale=(m == 8))
        probe, _ = prepared()
        out0 = probe.outliers()
        assert out0[1] > 0 and out0[3] > 0, out0
        g = slk.Msckf(mt, Pt)                                          # the same state received through the host
        rc, ng, ldg = nis_c(slk, g, FEAT, params, z, R)
        assert rc == 0
        np.testing.assert_array_equal(ng, n)
        np.testing.assert_array_equal(ldg, ld)


def test_usckf_nis_on_a_lower_only_P(slk):
    """Unit shape (N = 48): three lower-only steps, then slk_nis with nothing read out in between (launch_usckf completes
    P before an emission, too): the filter equals a twin that ran the steps alone, the numbers are numpy's on the
    emission of the same handle and those of a handle that received the state through the host."""
    B = 4
    s = sc.synthetic_usckf(B, seed=0x1E4B)

    def prepared():
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
        raw = RawCov(f)
        for _ in range(3):
            f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
        return f, raw
    z, R = np.ascontiguousarray(s["z"]), np.asarray(s["R"], dtype=np.float64)
    n, ld, (mt, Pt) = check_read_only_on_a_lower_only_P(
        slk, prepared, lambda f: nis_c(slk, f, VO, None, z, R), lambda f: innovation_device(slk, f, VO, None, z, R),
        3, "usckf-unit-shape", expect_stale=True)
    g = slk.Usckf(mean=mt, P=Pt, nfk=3, nfkl=9)
    rc, ng, ldg = nis_c(slk, g, VO, None, z, R)
    assert rc == 0
    np.testing.assert_array_equal(ng, n)
    np.testing.assert_array_equal(ldg, ld)


# ------------------------------------------------------------------ 3. a non-SPD S
@pytest.mark.parametrize("k,m", [(8, 8), (8, 32), (1, 6)])
def test_nis_with_a_non_spd_innovation_covariance(slk, k, m):
    """R = -0.3 I for filter 2 of 4 makes its S indefinite (test_msckf_update_with_a_non_spd_innovation_covariance): NaN /
    NaN for it, the other three finite and correct, no status bit, SLK_OK."""
    B = 4
    s, params, z, h = msckf_case(k, m, FEAT, B, seed=0x5BD + k + m)
    f = slk.Msckf(s["mean"], s["P"])
    R = np.repeat(0.01 * np.eye(m)[None], B, axis=0)
    R[2] = -0.3 * np.eye(m)
    X, Z = sigma_Z(f, h)
    Sn, nun = numpy_moments(Z, z, R)
    assert np.linalg.eigvalsh(Sn[2]).min() < 0
    rc, n, ld = nis_c(slk, f, FEAT, params, z, R)
    assert rc == 0
    assert np.isnan(n[2]) and np.isnan(ld[2])
    ok = [0, 1, 3]
    want_n, want_ld = reference(Sn[ok], nun[ok], ("non-spd", k, m))
    assert_stats(n[ok], ld[ok], want_n, want_ld, m, ("non-spd", k, m))
    assert (f.status() == 0).all()


# ------------------------------------------------------------------ 4. argument checks before any launch
def test_nis_argument_checks(slk):
    """The code slk_update_innovation returns for the same arguments, the filter bit-identical."""
    B, k, m = 2, 8, 8
    s = sc.synthetic_msckf(B, k, m=m, seed=0xBAD)
    f = slk.Msckf(s["mean"], s["P"])
    m0, P0 = state(f)
    lib = slk.load_library()
    X = f.update_sigma_points()
    Z = np.ascontiguousarray([[npc.mm_feature_proj(x, s["feat"][b]) for x in X[b]] for b in range(B)])
    bad_pose = s["feat"].copy()
    bad_pose[1, 0, 3] = k + 1
    m33 = 33
    cases = {
        "external without Z": (EXTERNAL, None, s["z"], s["R"], None),
        "Z without external": (FEAT, s["feat"], s["z"], s["R"], Z),
        "m > 32 on Msckf": (EXTERNAL, None, np.zeros((B, m33)), 0.01 * np.eye(m33), np.zeros((B, X.shape[1], m33))),
        "bad host pose index": (FEAT, bad_pose, s["z"], s["R"], None),
        "odd m": (FEAT, s["feat"], s["z"][:, :7], 0.01 * np.eye(7), None),
    }
    for what, (model, params, z, R, Zx) in cases.items():
        rc_i, _, _ = innovation(slk, f, model, params, z, R, Z=Zx)
        rc_n, n, ld = nis_c(slk, f, model, params, z, R, Z=Zx)
        assert rc_i != 0 and rc_n == rc_i, (what, rc_i, rc_n)
        assert (n == -7.0).all() and (ld == -7.0).all(), what
    rc, _, _ = nis_c(slk, f, FEAT, s["feat"], s["z"], s["R"], want_nis=False)            # NULL nis
    assert rc == slk.E_INVALID
    zc = np.ascontiguousarray(s["z"])
    assert lib.slk_nis(None, FEAT, None, 0, None, zc.ctypes.data, m, None, 0, zc.ctypes.data, None, slk.HOST) == slk.E_INVALID
    assert (f.status() == 0).all() and (f.outliers() == 0).all()
    m1, P1 = state(f)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_array_equal(P1, P0)


# ------------------------------------------------------------------ 5. slk_get_sigma
@pytest.mark.parametrize("kind", ["msckf", "usckf"])
def test_sigma_against_numpy(slk, kind):
    """Full range and a range that starts inside an SO(3) block, on the P that was set: rtol 4.5e-16 (two ulp: whether the
    device square root is correctly rounded is not established here); a planted negative diagonal entry gives NaN for
    that entry only."""
    B = 5
    if kind == "msckf":
        s = sc.synthetic_msckf(B, 8, m=8, seed=0x51)
        f = slk.Msckf(s["mean"], s["P"])
    else:
        s = sc.synthetic_usckf(B, seed=0x52)
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)
    N = f.N
    P = state(f)[1]
    want = np.sqrt(np.einsum("bii->bi", P))
    got = f.sigma()
    assert got.shape == (B, N)
    np.testing.assert_allclose(got, want, rtol=4.5e-16, atol=0)
    np.testing.assert_allclose(f.sigma(4, 9), want[:, 4:13], rtol=4.5e-16, atol=0)
    np.testing.assert_array_equal(f.sigma(N - 1), got[:, N - 1:])
    out = np.full((B, 3), -7.0)
    lib = slk.load_library()
    for t0, n in ((-1, 3), (0, 0), (N - 2, 3), (N, 1)):
        assert lib.slk_get_sigma(f._h, t0, n, out.ctypes.data, slk.HOST) == slk.E_INVALID
    assert lib.slk_get_sigma(f._h, 0, 3, None, slk.HOST) == slk.E_INVALID
    assert lib.slk_get_sigma(f._h, 0, 3, out.ctypes.data, 7) == slk.E_INVALID          # `where`
    assert (out == -7.0).all()
    Pn = P.copy()
    Pn[2, 7, 7] = -1e-3
    Pn[4, 0, 0] = np.nan
    f.set_state(None, Pn)
    got = f.sigma()
    bad = np.zeros((B, N), dtype=bool)
    bad[2, 7] = bad[4, 0] = True
    np.testing.assert_array_equal(np.isnan(got), bad)
    np.testing.assert_allclose(got[~bad], want[~bad], rtol=4.5e-16, atol=0)


@pytest.mark.parametrize("kind", ["msckf", "usckf"])
def test_sigma_reads_a_lower_only_covariance_as_it_is(slk, kind):
    """After three exact-shape steps P is lower-only.  The strict upper triangle in device memory is poisoned with NaN
    (through the pointer fetched BEFORE the steps: the address stays valid, nothing is completed by fetching it), then
    slk_get_sigma: equal to sqrt(diag) of a twin that ran the same steps, and the strict upper triangle in device memory
    is bit-unchanged (still the poison) across the call -- no mirror pass ran, the covariance is still lower-only.  The
    next read-out completes it: P equals the twin's."""
    import torch
    B = 4
    if kind == "msckf":
        s = sc.synthetic_msckf(B, 8, m=8, seed=0x53)
        new = lambda: slk.Msckf(s["mean"], s["P"])                                                         # noqa: E731
        step = lambda f: f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])  # noqa: E731
    else:
        s = sc.synthetic_usckf(B, seed=0x54)
        new = lambda: slk.Usckf(mean=s["mean"], P=s["P"], nfk=3, nfkl=9)                                    # noqa: E731
        step = lambda f: f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])    # noqa: E731
    f, twin = new(), new()
    N = f.N
    _, pP = f.device_pointers()                        # (complete here: nothing to mirror; the steps keep the buffer)
    for _ in range(3):
        step(f)
        step(twin)
    f.sync()
    # the handle's covariance buffer through the HIP runtime (column-major: element (i, j) at [b, j, i]), and the part of it
    # the lower-only steps leave stale: the strict upper triangle outside the 16 x 16 diagonal tiles
    import ctypes as C
    rt = C.CDLL("libamdhip64.so")

    def copy(dst, src, kind):                          # 1 = hipMemcpyHostToDevice, 2 = hipMemcpyDeviceToHost
        assert rt.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(B * N * N * 8), kind) == 0

    i, j = np.triu_indices(N, 1)
    keep = i // 16 != j // 16
    i, j = i[keep], j[keep]
    poisoned = np.empty((B, N, N))
    copy(poisoned.ctypes.data, pP, 2)
    poisoned[:, j, i] = np.nan
    copy(pP, poisoned.ctypes.data, 1)
    got = f.sigma()
    after = np.empty((B, N, N))
    copy(after.ctypes.data, pP, 2)
    assert after.tobytes() == poisoned.tobytes()                        # nothing written: the poison is still there
    assert np.isnan(after[:, j, i]).all()
    Pt = state(twin)[1]
    np.testing.assert_allclose(got, np.sqrt(np.einsum("bii->bi", Pt)), rtol=4.5e-16, atol=0)
    np.testing.assert_array_equal(got, twin.sigma())
    np.testing.assert_array_equal(state(f)[1], Pt)                      # the read-out mirrors the lower triangle over the poison
    dev = torch.empty((B, N), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert slk.load_library().slk_get_sigma(f._h, 0, N, dev.data_ptr(), slk.DEVICE) == 0
    f.sync()
    np.testing.assert_array_equal(dev.cpu().numpy(), got)


# ------------------------------------------------------------------ 6. Python Tier-B form and the C++ facade
def test_nis_functor_equals_the_registered_model(slk):
    B, k, m = 3, 2, 4
    s, params, z, h = msckf_case(k, m, FEAT, B, seed=0xF0C)
    f = slk.Msckf(s["mean"], s["P"])
    n, ld = f.nis(z, FEAT, params, s["R"], logdet=True)
    calls = iter(range(10 ** 9))
    per = 2 * f.N + 1
    nf, ldf = f.nis_functor(z, lambda x: npc.mm_feature_proj(x, s["feat"][next(calls) // per]), s["R"], logdet=True)
    np.testing.assert_allclose(nf, n, rtol=1e-9)
    np.testing.assert_allclose(ldf, ld, rtol=0, atol=1e-9 * m)
    np.testing.assert_array_equal(f.nis(z, FEAT, params, s["R"]), n)


def test_nis_through_cpp_facade(slk):
    """tests/cpp/nis_facade.cpp: nis(z, h, R) of the facade for registered models and host functors == numpy on the
    emitted sigma points of the same state through the Python package; the facade's filters are left as they were."""
    import facade_build
    res = facade_build.run(name="nis_facade")
    mean, P = res["msckf_mean"][:, 0][None], res["msckf_P"]
    f = slk.Msckf(mean, P[None])
    X = f.update_sigma_points()

    def check(name, Z, z, R):
        S, nu = numpy_moments(Z, z[None], R)
        want_n, want_ld = reference(S, nu, name)
        got = res[name][:, 0]
        assert_stats(got[:1], got[1:], want_n, want_ld, len(z), name)

    feat = res["msckf_feat"].T.reshape(1, -1, 4)
    zf = res["msckf_feat_z"][:, 0]
    check("msckf_feat_nis", np.array([[npc.mm_feature_proj(x, feat[0]) for x in X[0]]]), zf, 0.01 * np.eye(4))
    assert res["msckf_feat_nis_only"][0, 0] == res["msckf_feat_nis"][0, 0]
    zp = res["msckf_pose_z"][:, 0]
    check("msckf_pose_nis", np.array([[npc.mm_pose_position(x, 2) for x in X[0]]]), zp, 0.02 * np.eye(3))
    zq = res["msckf_functor_z"][:, 0]
    check("msckf_functor_nis", np.array([[np.concatenate([x[20:23], x[0:3]]) for x in X[0]]]), zq, 0.015 * np.eye(6))
    np.testing.assert_array_equal(res["msckf_mean_after"][:, 0], mean[0])
    np.testing.assert_array_equal(res["msckf_P_after"], P)
    assert res["msckf_status"][0, 0] == 0
    mean, P = res["usckf_mean"][:, 0][None], res["usckf_P"]
    g = slk.Usckf(mean=mean, P=P[None], nfk=3, nfkl=2)
    X = g.update_sigma_points()
    check("usckf_vo_nis", np.array([[npc.mm_vo_relative(x, 3) for x in X[0]]]), res["usckf_vo_z"][:, 0], 0.01 * np.eye(3))
    check("usckf_functor_nis", np.array([[np.array([x[39], x[39 + 3 + 1]]) for x in X[0]]]), res["usckf_functor_z"][:, 0],
          0.02 * np.eye(2))
    np.testing.assert_array_equal(res["usckf_P_after"], P)
    assert res["usckf_status"][0, 0] == 0
