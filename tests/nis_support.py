"""Helpers shared by tests/test_gpu_nis.py and tests/test_gpu_traj_diag.py: the C-ABI calls that have no Python wrapper, the
numpy reference of the innovation statistics and the comparison at the tolerances both files use (rtol 1e-9 on nis, atol
1e-9 * m on logdet, for cond(S) <= COND_MAX)."""
import numpy as np

COND_MAX = 1e4


# ------------------------------------------------------------------ helpers (the few lines of test_gpu_caller_gate.py)
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


def nis_c(slk, f, model, params, z, R, Z=None, want_nis=True, want_logdet=True):
    """slk_nis through the C ABI, host route -> (rc, nis [B], logdet [B]); the outputs start as a sentinel."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    B, m = z.shape
    pp, ps, _kp = _params(params)
    rp, rs, _kr = _R(R)
    Zc = None if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
    n, ld = np.full(B, -7.0), np.full(B, -7.0)
    rc = slk.load_library().slk_nis(f._h, model, pp, ps, None if Zc is None else Zc.ctypes.data, z.ctypes.data, m, rp, rs,
                                    n.ctypes.data if want_nis else None, ld.ctypes.data if want_logdet else None, slk.HOST)
    return rc, n, ld


def nis_device(slk, f, model, params, z, R):
    """f.nis with torch device tensors (where = SLK_DEVICE; matrices column-major per filter) -> numpy (nis, logdet)."""
    import torch
    dev = torch.device("cuda", 0)
    B, m = z.shape
    R = np.asarray(R, dtype=np.float64)
    Rc = R.T if R.ndim == 2 else np.transpose(R, (0, 2, 1))
    pt = None if params is None else torch.from_numpy(np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(B, -1))).to(dev)
    n, ld = f.nis(torch.from_numpy(np.ascontiguousarray(z)).to(dev), model, pt,
                  torch.from_numpy(np.ascontiguousarray(Rc)).to(dev), logdet=True)
    assert n.is_cuda and ld.is_cuda
    return n.cpu().numpy(), ld.cpu().numpy()


def sigma_Z(f, h):
    X = f.update_sigma_points()
    return X, np.ascontiguousarray([[h(b, x) for x in X[b]] for b in range(X.shape[0])])


def numpy_moments(Z, z, R):
    """meanSigmaPoints / covSigmaPoints + R (Msckf.hpp:234-238, Usckf.hpp:280-282): S [B, m, m], innovation [B, m]."""
    zbar = Z.mean(axis=1)
    D = Z - zbar[:, None, :]
    S = 0.5 * np.einsum("bpi,bpj->bij", D, D) + (R if R.ndim == 3 else R[None])
    return S, z - zbar


def reference(S, nu, what):
    """(nis, logdet) of numpy, after the condition on the inputs."""
    n, ld = np.empty(len(S)), np.empty(len(S))
    for b in range(len(S)):
        c = np.linalg.cond(S[b])
        assert c <= COND_MAX, (what, b, "cond(S_ref)", c)
        n[b] = nu[b] @ np.linalg.solve(S[b], nu[b])
        sign, ld[b] = np.linalg.slogdet(S[b])
        assert sign > 0, (what, b)
    return n, ld


def assert_stats(got_n, got_ld, want_n, want_ld, m, what):
    print(what, "nis rel err", float(np.max(np.abs(got_n - want_n) / np.abs(want_n))),
          "logdet abs err", float(np.max(np.abs(got_ld - want_ld))))
    np.testing.assert_allclose(got_n, want_n, rtol=1e-9, atol=0, err_msg=str(what))
    np.testing.assert_allclose(got_ld, want_ld, rtol=0, atol=1e-9 * m, err_msg=str(what))


def state(f):
    P = f.getPk() if hasattr(f, "getPk") else f.PkAugmentedState()
    return f.muState(), P
