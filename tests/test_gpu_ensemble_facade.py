"""slk_ensemble_moments / slk_gather_states through the raw forwarding forms of the C++ header facade
(tests/cpp/ensemble_facade.cpp) against the Python package and the numpy twin.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

from oracle import oracle as o
import ensemble_ref as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def test_ensemble_through_cpp_facade(slk):
    import facade_build
    res = facade_build.run(name="ensemble_facade")
    for kind in ("msckf", "usckf"):
        mean, truth, P = res[f"{kind}_mean"][:, 0][None], res[f"{kind}_truth"][:, 0][None], res[f"{kind}_P"][None]
        if kind == "msckf":
            lay = o.layout(o.MULTI, (mean.shape[1] - 13) // 7)
            f = slk.Msckf(mean, P)
        else:
            lay = o.layout(o.AUGMENTED, 0, 3, 2)
            f = slk.Usckf(mean=mean, P=P, nfk=3, nfkl=2)
        N = o.dof(lay)
        e = f.ensemble_moments(None, truth, 4, 5, ess=True)
        assert res[f"{kind}_bias"][:, 0].tobytes() == e["center"][0].tobytes()
        assert res[f"{kind}_espread"].tobytes() == e["spread"][0].tobytes()
        assert res[f"{kind}_ecov"].tobytes() == e["mean_cov"][0].tobytes()
        assert res[f"{kind}_ess"][0, 0] == 1.0
        np.testing.assert_allclose(res[f"{kind}_bias"][:, 0], o.boxminus(lay, truth[0], mean[0])[4:9], rtol=0, atol=1e-12)
        assert np.abs(res[f"{kind}_espread"]).max() <= 1e-24
        m = f.ensemble_moments(np.array([2.5]), None)
        assert res[f"{kind}_centre"][:, 0].tobytes() == m["center"][0].tobytes()
        assert res[f"{kind}_mspread"].tobytes() == m["spread"][0].tobytes()
        assert np.abs(o.boxminus(lay, res[f"{kind}_centre"][:, 0], mean[0])).max() <= 1e-12
        il = np.tril_indices(N)
        assert res[f"{kind}_mcov"][il].tobytes() == P[0][il].tobytes()
        assert res[f"{kind}_P_after"].tobytes() == P[0].tobytes()
        assert res[f"{kind}_refusals"][0, 0] == 7
        ref = er.moments(lay, mean, P, None, truth, 4, 5, 1)
        er.check_against_twin(lay, e, ref, True, kind + " facade")
