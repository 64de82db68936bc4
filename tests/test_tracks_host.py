"""Msckf feature-track update, the parts that need no GPU: the new exports and their declarations, the numpy twin's
Jacobian blocks against central differences of the oracle's own model and boxplus, its null space, the premise of the GPU
checks (the update does not depend on the basis of the null space), the flags of the constructed tracks, and the wrapper's
argument checks."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as o
import ekf_model_ref as ref
import tracks_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slk_track_linearize", "slk_update_tracks", "slk_step_tracks"]
GPU_TOL = 1e-9                                # TOL of tests/test_gpu_tracks.py


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from slkpkg import slk as mod
    return mod


def test_exports_in_library_and_wrapper(slk):
    lib = slk.load_library()
    for n in NEW:
        assert n in slk.EXPORTS and hasattr(lib, n), n
    for n in ("track_linearize", "update_tracks", "step_tracks"):
        assert hasattr(slk.Msckf, n)


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "slk.h")).read()
    for n in NEW:
        assert re.search(r"^int %s\(slk_filter \*f," % n, h, re.M), n
    assert "#define SLK_ABI_VERSION 1" in h
    assert "updateTracks" in open(os.path.join(ROOT, "include", "localization", "filters", "Msckf.hpp")).read()


@pytest.mark.parametrize("k,M,J,m", tr.SHAPES, ids=tr.IDS)
def test_twin_blocks_against_central_differences(k, M, J, m):
    # H_x: the oracle's mm_feature_proj with Lw = X composed with its boxplus; H_f: the same model differentiated in Lw.
    # Central differences with step 1e-6, bound 1e-6 max|H|: the comparison of tests/test_ekf_model_host.py
    s = tr.scenario(k, M, J, m)
    for b in range(min(2, s["B"])):
        for j in range(min(3, J)):
            X, flag, obs = tr.triangulate(s["mean"][b], s["tracks"][b, j])
            if flag != 1:
                continue
            r, Hx, Hf = tr.blocks(s["mean"][b], s["tracks"][b, j], X, obs, k)
            rows = np.concatenate([[2 * sl, 2 * sl + 1] for sl, _ in obs])
            feat = lambda Xw: np.array([[Xw[0], Xw[1], Xw[2], c] for _, c in obs])
            uv = np.concatenate([s["tracks"][b, j, sl, 1:3] for sl, _ in obs])
            np.testing.assert_allclose(r[rows], uv - ref.h_oracle(k, feat(X), s["mean"][b]), rtol=0, atol=1e-13)
            fd = ref.central_differences(k, feat(X), s["mean"][b])
            assert np.abs(fd - Hx[rows]).max() <= 1e-6 * np.abs(Hx).max(), (b, j)
            fdf = np.stack([(ref.h_oracle(k, feat(X + e), s["mean"][b]) - ref.h_oracle(k, feat(X - e), s["mean"][b])) / 2e-6
                            for e in 1e-6 * np.eye(3)], axis=1)
            assert np.abs(fdf - Hf[rows]).max() <= 1e-6 * np.abs(Hf).max(), (b, j)
            empty = np.setdiff1d(np.arange(2 * M), rows)
            assert not Hx[empty].any() and not Hf[empty].any() and not r[empty].any()
            Nn = np.linalg.qr(Hf, mode="complete")[0][:, 3:]
            assert np.abs(Nn.T @ Hf).max() <= 1e-13 * max(1.0, np.abs(Hf).max())


@pytest.mark.parametrize("shared", [False, True], ids=["per_filter", "shared"])
@pytest.mark.parametrize("k,M,J,m", tr.SHAPES, ids=tr.IDS)
def test_update_does_not_depend_on_the_basis(k, M, J, m, shared):
    # the premise of the GPU comparison: the oracle's EKF update on the twin's (r, H) and on the same rows multiplied per
    # track by a random orthogonal matrix agree within a tenth of the GPU tolerance; every filter uses a track
    s = tr.scenario(k, M, J, m, shared=shared)
    chi2 = tr.CHI2_95[:2 * M - 2]
    r, H, feat, gam = tr.linearize_batch(s, chi2)
    r2, H2, feat2, gam2 = tr.linearize_batch(s, chi2, rotate=np.random.default_rng(k * 100 + M))
    np.testing.assert_array_equal(feat, feat2)
    np.testing.assert_allclose(gam, gam2, rtol=1e-9)
    lay = o.layout(o.MULTI, k)
    for b in range(s["B"]):
        assert (feat[b, :, 3] == 1).any(), b
        for j in range(J):                                    # no gate decision hinges on rounding
            if np.isfinite(gam[b, j]):
                thr = chi2[2 * int((s["tracks"][b, j, :, 0] >= 0).sum()) - 3]
                assert abs(gam[b, j] - thr) > 1e-6 * thr
        fa, fb = o.Msckf(k, s["mean"][b], s["P"][b]), o.Msckf(k, s["mean"][b], s["P"][b])
        assert fa.update_ekf(r[b], np.zeros(m), H[b], np.eye(m), gate=False) == (0, 0)
        assert fb.update_ekf(r2[b], np.zeros(m), H2[b], np.eye(m), gate=False) == (0, 0)
        ep = float(np.abs(fa.P - fb.P).max() / np.abs(fa.P).max())
        em = float(np.abs(o.boxminus(lay, fa.mean, fb.mean)).max())
        print(f"k={k} M={M} b={b}: basis dependence P {ep:.2e}, mean {em:.2e}")
        assert ep <= 0.1 * GPU_TOL and em <= 0.1 * GPU_TOL, (b, ep, em)
        assert not np.array_equal(fa.P, s["P"][b])


def test_constructed_flags_and_gate_margins():
    s, s2, b = tr.flag_scenario()
    chi2 = tr.CHI2_95[:2 * s["M"] - 2]
    r, H, feat, gam = tr.linearize_batch(s2, chi2)
    assert feat[b, :5, 3].tolist() == [0, 0, -1, -1, -2], (feat[b, :5, 3], gam[b])
    assert (np.ascontiguousarray(feat[b, :2, :3]).view(np.uint64) == 0).all() and np.isnan(feat[b, 2:4, :3]).all()
    thr = chi2[2 * 5 - 3]
    assert gam[b, 4] > thr * (1 + 1e-6)
    nr = 2 * s["M"] - 3
    assert not r[b, :5 * nr].any() and not H[b, :5 * nr].any()
    # the mirrored track does triangulate -- behind the cameras
    obs = [(sl, int(c)) for sl, c in enumerate(s2["tracks"][b, 3, :, 0])]
    assert tr.triangulate(s2["mean"][b], s2["tracks"][b, 3])[1] == -1
    mirror = 2 * s["mean"][b, 0:3] - s["land"][b, 3]
    sp = tr.pose_offsets(obs[0][1])[0]
    assert (ref.quat_matrix(s["mean"][b, sp + 3:sp + 7]).T @ (mirror - s["mean"][b, sp:sp + 3]))[2] < 0


class _Fake:
    """Stands in for a filter where a wrapper must refuse before it touches the library."""
    B, N, Nq, KIND = 2, 24, 27, 1
    _lib = _h = None


def test_wrapper_argument_checks(slk):
    f = _Fake()
    f._track_args = lambda *a: slk.Msckf._track_args(f, *a)
    t = np.zeros((2, 4, 3, 3))
    with pytest.raises(slk.SlkError, match="tracks and sigma"):
        slk.Msckf.track_linearize(f, None, 0.01, 24)
    with pytest.raises(slk.SlkError, match="tracks and sigma"):
        slk.Msckf.update_tracks(f, t, None, 24)
    with pytest.raises(slk.SlkError, match="tracks must be"):
        slk.Msckf.track_linearize(f, np.zeros((3, 4, 3, 3)), 0.01, 24)
    with pytest.raises(slk.SlkError, match="tracks must be"):
        slk.Msckf.track_linearize(f, np.zeros((2, 4, 3, 2)), 0.01, 24)
    with pytest.raises(slk.SlkError, match="sigma must hold"):
        slk.Msckf.track_linearize(f, t, np.full(3, 0.01), 24)
    with pytest.raises(slk.SlkError, match="chi2 must hold"):
        slk.Msckf.track_linearize(f, t, 0.01, 24, chi2=np.ones(3))
