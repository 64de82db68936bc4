"""The reference side of the Msckf EKF update tests (tests/test_gpu_ekf.py), without a GPU: the C oracle against the
independent numpy twin (oracle/np_check.py) and the textbook update, on the scenarios the GPU tests hold the kernels
to -- a dense full-rank Jacobian, outliers pinned by place, m = 512 and the known answers -- plus the host-side
refusals of the Python wrapper."""
import numpy as np
import pytest

from oracle import np_check as npc
from oracle import oracle as o
import scenarios as sc

TOL = 1e-11


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def oracle_and_numpy(e, b, gate=True, tol=TOL):
    """Filter b through the oracle and the numpy twin: the same status, outliers and state -> (status, outliers,
    oracle filter, the twin's gate d2 values)."""
    k = e["k"]
    f = o.Msckf(k, e["mean"][b], e["P"][b])
    st, no = f.update_ekf(e["z"][b], e["zmean"][b], e["H"][b], e["R"][b], gate=gate)
    h = npc.Msckf(k, e["mean"][b], e["P"][b])
    d2 = []
    no2, flag = npc.msckf_update_ekf(h, e["z"][b], e["zmean"][b], e["H"][b], e["R"][b], gate=gate, decisions=d2)
    assert no2 == no and st in (0, 16) and (flag == "rows") == (st == 16), (st, no, no2, flag)
    lay = o.layout(o.MULTI, k)
    assert rel(f.P, h.P) <= tol and float(np.abs(o.boxminus(lay, f.mean, h.mean)).max()) <= tol
    return st, no, f, d2


@pytest.mark.parametrize("k,m", [(0, 12), (2, 40), (8, 60), (8, 128), (9, 80), (8, 130)])
def test_ekf_dense_jacobian_oracle_and_numpy_agree(k, m):
    e = sc.synthetic_ekf(2, k, m, seed=0xDE5E + k + m, dense=True)
    for b in range(2):
        oracle_and_numpy(e, b)
        oracle_and_numpy(e, b, gate=False)


@pytest.mark.parametrize("case", sc.EKF_EDGE_CASES)
@pytest.mark.parametrize("m", [128, 160])
def test_ekf_gate_edges_on_the_reference(m, case):
    # the GPU test's inputs: the pinned rejection counts, decisions far from the threshold, no update where m' < N or 0
    e = sc.ekf_gate_edge(3, 8, m, case, seed=0xED6E + m)
    N = e["N"]
    left = m - 2 * e["n_out"]
    for b in range(3):
        st, no, f, d2 = oracle_and_numpy(e, b)
        assert no == e["n_out"] and st == (16 if 0 < left < N else 0), (no, st)
        assert np.abs(np.array(d2) - 5.99).min() / 5.99 > 1e-6
        if st or left == 0:
            assert np.array_equal(f.P, e["P"][b]) and np.array_equal(f.mean, e["mean"][b])
        else:
            assert rel(f.P, e["P"][b]) > 1e-6


@pytest.mark.parametrize("k", [9, 33])
def test_ekf_512_rows_oracle_and_numpy_agree(k):
    e = sc.synthetic_ekf(2, k, 512, seed=0x5120 + k, dense=True)      # the GPU test's filters
    for b in range(2):
        st, no, _, _ = oracle_and_numpy(e, b, tol=1e-10)
        assert st == 0 and no > 0


@pytest.mark.parametrize("k,m,iso", [(8, 60, False), (8, 128, True), (9, 80, True), (9, 66, False)])
def test_ekf_known_answers_on_the_reference(k, m, iso):
    # gate off, dense H: m = N with a non-isotropic R, or R = s^2 I -- the textbook update (the GPU test's inputs)
    B = 3
    e = sc.synthetic_ekf(B, k, m, seed=0x7E47 + k + m, outliers=False, dense=True)
    if iso:
        e["R"] = np.ascontiguousarray(np.broadcast_to(0.04 * np.eye(m), (B, m, m)))
    lay = o.layout(o.MULTI, k)
    for b in range(B):
        st, no, f, _ = oracle_and_numpy(e, b, gate=False)
        assert st == 0 and no == 0
        Hb, Pb = e["H"][b], e["P"][b]
        S = Hb @ Pb @ Hb.T + e["R"][b]
        K = Pb @ Hb.T @ np.linalg.inv(S)
        assert rel(f.P, Pb - K @ S @ K.T) <= 1e-10
        mu = o.boxplus(lay, e["mean"][b], K @ (e["z"][b] - e["zmean"][b]))
        assert float(np.abs(o.boxminus(lay, f.mean, mu)).max()) <= 1e-10


def test_wrapper_marshalling_refuses_bad_tensors_on_the_host():
    # the helpers every update path marshals through raise SlkError (not a bare assert) before any library call
    torch = pytest.importorskip("torch")
    from slkpkg import slk
    B, m = 2, 4
    z = torch.zeros((B, m), dtype=torch.float64)
    with pytest.raises(slk.SlkError, match="zmean"):
        slk._zrows(z.float(), B, m, "zmean")
    with pytest.raises(slk.SlkError):
        slk._zrows(torch.zeros((m, B), dtype=torch.float64).t(), B, m)           # not contiguous
    with pytest.raises(slk.SlkError):
        slk._zrows(z, B, m + 1)                                                   # wrong size
    with pytest.raises(slk.SlkError):
        slk._mat(torch.eye(m, dtype=torch.float32), B, m)
    with pytest.raises(slk.SlkError):
        slk._mat(torch.zeros((1, m, m), dtype=torch.float64), B, m)
    host = slk._zrows(np.zeros((B, m)), B, m)
    assert slk._where(host, slk._zrows(z, B, m)) == slk.HOST                     # a CPU tensor is host memory
    with pytest.raises(slk.SlkError, match="same side"):
        slk._where(host, slk._Arg(1, m, slk.DEVICE, None))
