"""GPU test of the facade's feature-track update (include/localization/filters/Msckf.hpp): the client
tests/cpp/tracks_facade.cpp runs updateTracks(tracks, sigma[, chi2]); its posteriors, flags and points against the Python
route on the same inputs (the same library: bit for bit) and against the CPU oracle on the numpy twin's rows."""
import numpy as np
import pytest

from oracle import oracle as o
import tracks_ref as tr

pytestmark = pytest.mark.gpu
TOL = 1e-9                                    # the tolerance of the EKF update (tests/test_gpu_ekf.py)
K, N, J, M, m = 2, 24, 8, 3, 24


@pytest.fixture(scope="module")
def res():
    import __graft_entry__ as ge
    ge.build()
    import facade_build
    return facade_build.run(name="tracks_facade")


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    return mod


def inputs(res):
    return res["mean0"][:, 0], res["P0"], np.ascontiguousarray(res["tracks"].T).reshape(1, J, M, 3), res["chi2"][0]


@pytest.mark.parametrize("form", ["plain", "gated"])
def test_facade_equals_python_route(res, slk, form):
    mean0, P0, tracks, chi2 = inputs(res)
    f = slk.Msckf(mean0[None], P0[None])
    feat = f.update_tracks(tracks, tr.SIGMA, m, chi2=chi2 if form == "gated" else None)
    np.testing.assert_array_equal(res[f"{form}_flags"][:, 0], feat[0, :, 3])
    np.testing.assert_array_equal(res[f"{form}_feat"].T, feat[0])
    np.testing.assert_array_equal(res[f"{form}_mean"][:, 0], f.muState()[0])
    np.testing.assert_array_equal(res[f"{form}_P"], f.getPk()[0])
    assert list(res["status"][:, 0]) == [0, 0]
    want = [1, 1, 1, 1, 1, 0, 1, 1] if form == "plain" else [1, 1, 1, 1, 1, 0, -2, 1]
    assert feat[0, :, 3].tolist() == want


@pytest.mark.parametrize("form", ["plain", "gated"])
def test_facade_against_the_oracle(res, form):
    mean0, P0, tracks, chi2 = inputs(res)
    c2 = chi2 if form == "gated" else None
    r, H, feat, gam = tr.linearize_np(mean0, P0, tracks[0], tr.SIGMA, K, m, c2)
    if c2 is not None:
        assert np.all(np.abs(gam[np.isfinite(gam)] - c2[3]) > 1e-6 * c2[3]), gam
    np.testing.assert_array_equal(feat[:, 3], res[f"{form}_flags"][:, 0])
    ref = o.Msckf(K, mean0, P0)
    assert ref.update_ekf(r, np.zeros(m), H, np.eye(m), gate=False) == (0, 0)
    lay = o.layout(o.MULTI, K)
    ep = float(np.abs(res[f"{form}_P"] - ref.P).max() / np.abs(ref.P).max())
    em = float(np.abs(o.boxminus(lay, res[f"{form}_mean"][:, 0], ref.mean)).max())
    assert ep <= TOL and em <= TOL, (ep, em)
    assert not np.array_equal(res[f"{form}_P"], P0)
