"""slk_gather_states on the device (csrc/slk_ensemble.hpp): filter b becomes the old filter src[b], bit for bit what
slk_get_state, a host index and slk_set_state give, with a complete and with a lower-only covariance, on every shape of
tests/ensemble_ref.py; then the loop weight -> estimate -> resample once.  Every case here fails without the call.  Run
with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

from oracle import oracle as o
import scenarios as sc
import ensemble_ref as er

pytestmark = pytest.mark.gpu

def batch_of(name):
    return er.SHAPES[er.SHAPE_IDS.index(name)][3]         # the shapes' own batch sizes, as in the moments tests


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


def step(slk, b, f, s):
    """one slk_step (Msckf) or predict + update (Usckf)"""
    if b["kind"] == "msckf":
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    else:
        f.predict(slk.PM_CONST_VELOCITY, s["u"], s["Q"])
        f.update(s["z"], slk.MM_VO_RELATIVE, None, s["R"], gate=0)


def index_sets(B, rng):
    return {"identity": np.arange(B), "permutation": rng.permutation(B), "from_one": np.full(B, B // 3),
            "repeats": rng.integers(0, B, B)}


def tag_status(slk, f, b, s):
    """give the filters different status words and outlier counts: a gated two-feature update whose measurements are far
    off on every third filter (blocks of two rows, which the chi-square gate covers at every shape)"""
    if b["kind"] == "msckf":
        feat, z = s["feat"][:, :2], s["z"][:, :4].copy()
    else:
        feat, z = sc.usckf_features(b["mean"], poses=(0, 2))
    z[::3] += 50.0
    f.update(z, slk.MM_FEATURE_PROJ, feat, 0.01 * np.eye(4), gate=1)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("name", er.SHAPE_IDS)
def test_gather_equals_host_index(slk, name, route):
    import torch
    B = batch_of(name)
    b, s = er.step_inputs(name, 4, B)
    rng = np.random.default_rng(0x6A7)
    for what, src in index_sets(B, rng).items():
        f = make_filter(slk, b)
        tag_status(slk, f, b, s)
        mean, P, st, oc = snapshot(f)
        assert len(set(st.tolist())) > 1 and len(set(oc.tolist())) > 1, (name, "the filters carry no distinct status / outliers")
        ptrs = f.device_pointers()
        f.gather(src if route == "host" else torch.from_numpy(src.astype(np.int32)).to("cuda:0"))
        assert f.device_pointers() != ptrs, what
        rm, rP, rs, ro = er.gather(mean, P, st, oc, src)
        gm, gP, gs, go = snapshot(f)
        assert gm.tobytes() == rm.tobytes() and gP.tobytes() == rP.tobytes(), (name, what)
        assert gs.tobytes() == rs.tobytes() and go.tobytes() == ro.tobytes(), (name, what)
        # the next step == the same step on a handle given the gathered state through set_state
        g = make_filter(slk, b, rm, rP)
        step(slk, b, f, s)
        step(slk, b, g, s)
        am, aP, _, ao = snapshot(f)
        bm, bP, _, bo = snapshot(g)
        assert am.tobytes() == bm.tobytes() and aP.tobytes() == bP.tobytes() and ao.tobytes() == bo.tobytes(), (name, what)


@pytest.mark.parametrize("name", ["msckf_n60", "usckf_n48"])
def test_gather_of_a_lower_only_covariance(slk, name):
    """after the exact-shape steps P is lower-only: it is gathered as its lower triangle and stays lower-only"""
    B = batch_of(name)
    b, s = er.step_inputs(name, 4, B)

    def stepped():
        f = make_filter(slk, b)
        for _ in range(2):
            if b["kind"] == "msckf":
                f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
            else:
                f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
        return f

    mean, P, st, oc = snapshot(stepped())
    for what, src in index_sets(B, np.random.default_rng(0x10E)).items():
        f = stepped()
        f.gather(src)
        rm, rP, rs, ro = er.gather(mean, P, st, oc, src)
        g = make_filter(slk, b, rm, rP)
        step(slk, b, f, s)                                   # (straight on the gathered lower-only covariance)
        step(slk, b, g, s)
        am, aP, _, ao = snapshot(f)
        bm, bP, _, bo = snapshot(g)
        assert am.tobytes() == bm.tobytes() and aP.tobytes() == bP.tobytes() and ao.tobytes() == bo.tobytes(), (name, what)
        f = stepped()
        f.gather(src)
        gm, gP, gs, go = snapshot(f)
        assert gm.tobytes() == rm.tobytes() and gP.tobytes() == rP.tobytes(), (name, what)
        assert gs.tobytes() == rs.tobytes() and go.tobytes() == ro.tobytes(), (name, what)


def test_bad_indices(slk):
    import torch
    B = 16
    b, s = er.step_inputs("msckf_n60", 4, B)
    f = make_filter(slk, b)
    before = snapshot(f)
    ptrs = f.device_pointers()
    for bad in (-1, B, 2 ** 31 - 1):
        src = np.arange(B)
        src[5] = bad
        with pytest.raises(slk.SlkError, match="slk_gather_states failed with code -1"):
            f.gather(src)
    assert f._lib.slk_gather_states(f._h, None, slk.HOST) == slk.E_INVALID
    assert f._lib.slk_gather_states(f._h, np.arange(B, dtype=np.int32).ctypes.data, 7) == slk.E_INVALID
    for x, y in zip(before, snapshot(f)):
        assert x.tobytes() == y.tobytes()
    assert f.device_pointers() == ptrs
    # device-resident indices: the filter keeps its own state and gets ST_BAD_INDEX, the others are gathered
    src = np.random.default_rng(3).integers(0, B, B).astype(np.int32)
    src[[2, 9]] = [-4, B]
    f.gather(torch.from_numpy(src).to("cuda:0"))
    ok = src.copy()
    ok[[2, 9]] = [2, 9]
    gm, gP, gs, go = snapshot(f)
    assert gm.tobytes() == before[0][ok].tobytes() and gP.tobytes() == before[1][ok].tobytes()
    want = before[2][ok].copy()
    want[[2, 9]] |= slk.ST_BAD_INDEX
    assert (gs == want).all() and (go == before[3][ok]).all()


def test_weight_estimate_resample_loop(slk):
    """nis -> weights -> ensemble_moments -> indices from torch.searchsorted -> gather, nothing leaving the device; the
    moments after the gather with uniform weights equal the twin on the gathered states"""
    import torch
    B, G = 512, 1
    b, s = er.step_inputs("msckf_n60", G, B)
    lay = b["lay"]
    f = make_filter(slk, b)
    dev = torch.device("cuda", 0)
    z, feat, R = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (s["z"], s["feat"].reshape(B, -1), s["R"]))
    nis, logdet = f.nis(z, slk.MM_FEATURE_PROJ, feat, R, logdet=True)
    loglik = -0.5 * (nis + logdet + s["m"] * np.log(2 * np.pi))
    w = torch.exp(loglik - loglik.max()).contiguous()
    est = f.ensemble_moments(w, None, 0, 6, ess=True)
    assert est["center"].is_cuda and 1.0 <= float(est["ess"][0]) <= B
    ref = er.moments(lay, b["mean"], b["P"], w.cpu().numpy(), None, 0, 6, G)
    er.check_against_twin(lay, {k: v.cpu().numpy() for k, v in est.items()}, ref, False, "weighted estimate")
    # systematic resampling
    cdf = torch.cumsum(w / w.sum(), 0)
    u = (torch.arange(B, dtype=torch.float64, device=dev) + 0.5) / B
    src = torch.clamp(torch.searchsorted(cdf, u), max=B - 1).to(torch.int32).contiguous()
    f.gather(src)
    idx = src.cpu().numpy()
    gm, gP = f.muState(), f._getP()
    assert gm.tobytes() == b["mean"][idx].tobytes() and gP.tobytes() == b["P"][idx].tobytes()
    after = f.ensemble_moments(None, None, 0, 6, ess=True)
    er.check_against_twin(lay, after, er.moments(lay, gm, gP, None, None, 0, 6, G), False, "after the gather")
