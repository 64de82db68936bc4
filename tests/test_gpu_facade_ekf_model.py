"""GPU test of the facade's EKF update from a registered model (include/localization/filters/Msckf.hpp): the client
tests/cpp/ekf_model_facade.cpp runs update(z, slk::FeatureProjectionModel, H, R) next to the functor form with a
hand-written Jacobian and next to the caller-gated form; all three against each other and against the CPU oracle."""
import numpy as np
import pytest

from oracle import oracle as o
import ekf_model_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-9                                    # the tolerance of the EKF update (tests/test_gpu_ekf.py)
K, N, M = 2, 24, 28


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.fixture(scope="module")
def res():
    import __graft_entry__ as ge
    ge.build()
    import facade_build
    return facade_build.run(name="ekf_model_facade")


def test_model_form_equals_functor_form(res):
    lay = o.layout(o.MULTI, K)
    assert list(res["status"][:, 0]) == [0, 0, 0]
    assert list(res["outliers"][:, 0]) == [1, 1, 1]
    for other in ("functor", "custom"):
        assert rel(res["model_P"], res[f"{other}_P"]) <= TOL
        assert np.abs(o.boxminus(lay, res["model_mean"][:, 0], res[f"{other}_mean"][:, 0])).max() <= TOL
    assert not np.array_equal(res["model_P"], res["P0"])


def test_jacobians_through_the_facade(res):
    # the device form leaves the caller's H alone; the caller-gated form fills it with the device linearisation, which
    # agrees with the client's hand-written Jacobian to the 1e-12 of tests/test_gpu_ekf_model.py
    assert (res["model_H"] == -7.0).all()
    assert np.abs(res["custom_H"] - res["functor_H"]).max() <= 1e-12 * max(1.0, np.abs(res["functor_H"]).max())
    assert (res["custom_H"][:, 6:12] == 0).all()


def test_model_form_against_the_oracle(res):
    # the oracle on the client's own h(mu) and H
    lay = o.layout(o.MULTI, K)
    mean0, P0, H = res["mean0"][:, 0], res["P0"], res["functor_H"]
    assert H.shape == (M, N) and np.linalg.matrix_rank(H) == 6 * (K + 1)
    # z and the landmarks are not printed: rebuild them as the client does
    nf = M // 2
    feat, z = np.zeros((1, nf, 4)), np.zeros(M)
    for f in range(nf):
        pose = f % (K + 1)
        sp = 0 if pose == 0 else 13 + 7 * (pose - 1)
        l = np.array([0.8 * np.sin(1.7 * f), 0.8 * np.cos(2.3 * f), 4.0 + 3.0 * abs(np.sin(0.9 * f))])
        feat[0, f, :3] = mean0[sp:sp + 3] + ref.quat_matrix(mean0[sp + 3:sp + 7]) @ l
        feat[0, f, 3] = pose
        z[2 * f], z[2 * f + 1] = l[0] / l[2] + 0.03 * np.sin(3.1 * f), l[1] / l[2] + 0.03 * np.cos(1.9 * f)
    z[10] += 25.0
    zm, Hn = ref.linearize_np(mean0[None], feat, K)
    assert np.abs(Hn[0] - H).max() <= 1e-12                   # the same features as the client's
    R = 0.01 * np.eye(M)
    d2 = ref.gate_d2(K, mean0, P0, z, zm[0], Hn[0], R)
    assert np.all(np.abs(d2 - ref.CHI2) > 1e-6), d2
    r = o.Msckf(K, mean0, P0)
    st, no = r.update_ekf(z, zm[0], Hn[0], R, gate=True)
    assert (st, no) == (0, 1)
    assert rel(res["model_P"], r.P) <= TOL
    assert np.abs(o.boxminus(lay, res["model_mean"][:, 0], r.mean)).max() <= TOL
