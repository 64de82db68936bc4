"""EKF update from registered models, the parts that need no GPU: the new exports and their declarations, the numpy
reference Jacobian of the GPU tests against central differences of the oracle's own model and boxplus, the premises of
the oracle comparison (gate margins, rank of H), and the wrapper's argument checks."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as o
import ekf_model_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slk_ekf_linearize", "slk_update_ekf_model", "slk_step_ekf", "slk_step_n_ekf"]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from slkpkg import slk as mod
    return mod


def test_exports_in_library_and_wrapper(slk):
    lib = slk.load_library()
    for n in NEW:
        assert n in slk.EXPORTS and hasattr(lib, n), n


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "slk.h")).read()
    for n in NEW:
        assert re.search(r"^int %s\(slk_filter \*f," % n, h, re.M), n
    assert "#define SLK_ABI_VERSION 1" in h


@pytest.mark.parametrize("k,m", ref.SHAPES, ids=[f"k{k}-m{m}" for k, m in ref.SHAPES])
def test_numpy_jacobian_against_central_differences(k, m):
    # central differences with step h = 1e-6: truncation ~ h^2 |h'''|, rounding ~ eps / h ~ 1e-10; bound 1e-6 max|H|
    s = ref.scenario(k, m)
    zmean, H = ref.linearize_np(s["mean"], s["feat"], k)
    for b in range(s["B"]):
        np.testing.assert_allclose(zmean[b], ref.h_oracle(k, s["feat"][b], s["mean"][b]), rtol=0, atol=1e-13)
        fd = ref.central_differences(k, s["feat"][b], s["mean"][b])
        err = np.abs(fd - H[b]).max()
        print(f"k={k} m={m} b={b}: max |dH| {err:.2e}, max |H| {np.abs(H[b]).max():.2e}")
        assert err <= 1e-6 * np.abs(H[b]).max(), (b, err)
        assert not H[b][:, 6:12].any()


@pytest.mark.parametrize("outliers", [False, True], ids=["clean", "outliers"])
@pytest.mark.parametrize("k,m", ref.SHAPES[:5], ids=[f"k{k}-m{m}" for k, m in ref.SHAPES[:5]])
def test_premises_of_the_oracle_comparison(k, m, outliers):
    # what tests/test_gpu_ekf_model.py relies on for these seeds: no gate decision within 1e-6 of the threshold in ANY
    # filter, and H of full rank on its non-zero columns (6 per distinct observed pose) with sigma_min / sigma_max > 1e-6
    s = ref.scenario(k, m, outliers=outliers)
    zmean, H = ref.linearize_np(s["mean"], s["feat"], k)
    for b in range(s["B"]):
        d2 = ref.gate_d2(k, s["mean"][b], s["P"][b], s["z"][b], zmean[b], H[b], s["R"])
        assert d2.size and np.all(np.abs(d2[np.isfinite(d2)] - ref.CHI2) > 1e-6), (b, d2)
        rank, poses, ratio = ref.rank_premise(H[b])
        assert poses == len(set(s["feat"][b, :, 3])) and rank == 6 * poses and ratio > 1e-6, (b, rank, poses, ratio)
        r = o.Msckf(k, s["mean"][b], s["P"][b])
        st, no = r.update_ekf(s["z"][b], zmean[b], H[b], s["R"], gate=True)
        if not outliers:
            assert st == 0 and np.isfinite(r.P).all() and np.linalg.eigvalsh(0.5 * (r.P + r.P.T)).min() > 0, (b, st, no)


class _Fake:
    """Stands in for a filter where a wrapper must refuse before it touches the library."""
    B, N, Nq, KIND = 2, 12, 13, 1
    _lib = _h = None

    def _default_gate(self, gate):
        return 1


def test_wrapper_argument_checks(slk):
    f = _Fake()
    f._model_params = lambda *a: slk.Msckf._model_params(f, *a)
    z = np.zeros((2, 12))
    with pytest.raises(slk.SlkError, match="parameters"):
        slk.Msckf.ekf_linearize(f, slk.MM_FEATURE_PROJ, None, 12)
    with pytest.raises(slk.SlkError, match="parameters"):
        slk.Msckf.update_ekf_model(f, z, slk.MM_FEATURE_PROJ, None, np.eye(12))
    with pytest.raises(slk.SlkError, match="parameters"):
        slk.Msckf.step_ekf(f, slk.PM_DELTA_POSE, np.zeros(13), np.eye(12), z, slk.MM_FEATURE_PROJ, None, np.eye(12))
    with pytest.raises(slk.SlkError, match="'ukf' or 'ekf'"):
        slk.Msckf.step_n(f, slk.PM_DELTA_POSE, np.zeros((1, 13)), np.eye(12), z[None], slk.MM_FEATURE_PROJ, None, np.eye(12),
                         update="eks")
    with pytest.raises(AssertionError):                       # a parameter row shorter than (m / 2) x 4
        slk.Msckf.ekf_linearize(f, slk.MM_FEATURE_PROJ, np.zeros((2, 20)), 12)
