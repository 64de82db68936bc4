"""Msckf predict with two filters per wave (csrc/slk_kernels.hpp: msckf_predict_pair_kernel) against the one-wave kernel.

From slk.PREDICT_PAIR_MIN_BATCH filters on the plain predict route (registered process model, no sigma-point emission) runs
the pair kernel; below it msckf_predict_kernel.  Filters are independent of their batch, and the pair kernel claims the same
operations on the same operands in the same order, so the reference of every case is the SAME filter run in a batch below the
threshold, and the comparison is bit for bit on mean, P and status (NaNs included: the arrays are compared as 64-bit words).

A small set of filters is run once per case in batches below the threshold (one-wave kernel; in chunks, whatever the
threshold's value) and then tiled over a batch at or above it, filter i of the large batch = filter i mod n of the set with n
odd: every filter of the set sits in the lower half of some wave and in the upper half of another, and every ordered pair of
neighbours (i, i + 1 mod n) shares a wave.

The k = 0 set (N = 12, seven filters):
  0, 5, 6  the synthetic scale (two passes of the mean loop);
  1        a rotation block of order 1 rad^2 -- more passes, sigma rotations beyond the series' domain;
  2        a rotation block of order 1e-8 rad^2 -- it shares its wave with filter 1 (pairs (1, 2) and (2, 3));
  3        a 12 x 12 block that is not positive definite, 4 one with a NaN: SLK_ST_LLT_FAIL, mean and P unchanged, while their
           partners (2, 4 / 3, 5) match their unpaired results.
Cases: each process model x shared and per-filter Q (q_stride 0 / 144), predict-only, on a large ODD batch (the last filter alone
in its wave), a large even one, the threshold itself (the smallest batch of the pair route) and the threshold + 1; a two-step
step_n beyond 4096 filters (k = 0 launches predict on its own there: the launch site of launch_msckf); a full step and a
two-step step_n at k = 8 / m = 8 on the smallest batch of the pair route and on an odd batch of 257 (the launch site of the
N = 49 .. 64 step).  That nothing behind filter B - 1 is written on an odd batch is checked where guard words
can be placed: slk_selftest_predict_pair, on arrays of its own.
Run with `pytest -m gpu` on an MI355X.
"""
import numpy as np
import pytest

import scenarios as sc

pytestmark = pytest.mark.gpu
NSET = 7
BIG = 2048              # the large batches: two rounds of pair waves on the chip's 1024 SIMDs would be 4096; one is enough here


def chunks(n, slk):
    """Index blocks of at most PREDICT_PAIR_MIN_BATCH - 1 filters: batches the one-wave kernel serves."""
    size = min(n, slk.PREDICT_PAIR_MIN_BATCH - 1)
    assert size >= 1
    return [np.arange(i, min(n, i + size)) for i in range(0, n, size)]


def batch_of(slk, which):
    T = slk.PREDICT_PAIR_MIN_BATCH
    return {"big_odd": max(T, BIG) + 1 + (max(T, BIG) & 1), "big_even": max(T, BIG) + (max(T, BIG) & 1), "smallest": T,
            "smallest_plus_one": T + 1}[which]


@pytest.fixture(scope="module")
def slk():
    import torch  # noqa: F401  (loads the HIP runtime the library binds to)
    from slkpkg import slk as mod
    assert mod.device_count() > 0, "no MI355X visible"
    return mod


def words(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    g, w = words(got), words(want)
    bad = np.argwhere((g != w).reshape(g.shape[0], -1).any(axis=1)).ravel()
    assert bad.size == 0, f"{what}: filters {bad[:8].tolist()} of {g.shape[0]} differ ({bad.size} in all)"


def small_set():
    """The seven k = 0 filters of the module docstring."""
    s = sc.synthetic_msckf(NSET, 0, m=8, seed=0x9A1B0000)
    P = s["P"].copy()
    P[1, 3:6, 3:6] += np.eye(3)                                  # order 1 rad^2
    d = np.ones(12)
    d[3:6] = 1e-3
    P[2] = P[2] * d[:, None] * d[None, :]                        # a congruence: still SPD, rotation block 1e-8 rad^2
    P[3, 5, 5] = -1.0                                            # not positive definite
    P[4, 2, 1] = P[4, 1, 2] = np.nan
    s["P"] = np.ascontiguousarray(P)
    rng = np.random.default_rng(0x9A1B0001)
    u_cv = np.concatenate([rng.normal(0.1, 0.02, (NSET, 3)), rng.normal(0.0, 0.05, (NSET, 3)), np.full((NSET, 1), 0.1)], axis=1)
    u_dr = np.concatenate([np.full((NSET, 1), 0.1), rng.normal(0.5, 0.1, (NSET, 3)), rng.normal(0.0, 0.1, (NSET, 3)),
                           rng.normal(0.5, 0.1, (NSET, 3)), rng.normal(0.0, 0.1, (NSET, 3))], axis=1)
    s["u_by_model"] = {"cv": np.ascontiguousarray(u_cv), "dp": s["u"], "dr": np.ascontiguousarray(u_dr)}
    return s


@pytest.fixture(scope="module")
def kset():
    return small_set()


def model_of(slk, name):
    return {"cv": slk.PM_CONST_VELOCITY, "dp": slk.PM_DELTA_POSE, "dr": slk.PM_DEAD_RECKON}[name]


def q_of(s, per_filter, idx):
    if not per_filter:
        return s["Q"]
    return np.ascontiguousarray(s["Q"][None] * (1.0 + 0.25 * idx)[:, None, None])


def predict_once(slk, s, model, per_filter_q, idx):
    """One predict of filters idx (indices into the set) -> mean, P, status."""
    f = slk.Msckf(s["mean"][idx], s["P"][idx])
    f.predict(model_of(slk, model), s["u_by_model"][model][idx], q_of(s, per_filter_q, idx))
    out = f.muState(), f.getPk(), f.status()
    f.close()
    return out


_REF = {}


def reference(slk, s, model, per_filter_q):
    """The one-wave kernel's result for the set (batches below the threshold), computed once per case and left alone."""
    key = (model, per_filter_q)
    if key not in _REF:
        parts = [predict_once(slk, s, model, per_filter_q, c) for c in chunks(NSET, slk)]
        _REF[key] = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    return _REF[key]


def check_reference_is_what_the_case_says(slk, s, ref):
    mean, P, st = ref
    assert st.tolist() == [0, 0, 0, slk.ST_LLT_FAIL, slk.ST_LLT_FAIL, 0, 0], st
    for b in (3, 4):                                             # a failed factorisation leaves the filter unchanged
        same_bits(mean[b:b + 1], s["mean"][b:b + 1], f"one-wave kernel, failed filter {b}: mean")
        same_bits(P[b:b + 1], s["P"][b:b + 1], f"one-wave kernel, failed filter {b}: P")
    for b in (0, 1, 2, 5, 6):
        assert np.isfinite(P[b]).all() and np.isfinite(mean[b]).all()
        assert (words(P[b]) != words(s["P"][b])).any()


@pytest.mark.parametrize("per_filter_q", [False, True], ids=["Qshared", "Qperfilter"])
@pytest.mark.parametrize("model", ["cv", "dp", "dr"])
@pytest.mark.parametrize("which", ["big_odd", "big_even", "smallest", "smallest_plus_one"])
def test_predict_only_pairs_match_the_one_wave_kernel(slk, kset, model, per_filter_q, which):
    B = batch_of(slk, which)
    assert B >= slk.PREDICT_PAIR_MIN_BATCH
    ref = reference(slk, kset, model, per_filter_q)
    check_reference_is_what_the_case_says(slk, kset, ref)
    idx = (np.arange(B) + 1) % NSET                             # (filters 1 and 2 share the first wave of every batch)
    if which.startswith("big"):
        assert (B % 2 == 1) == (which == "big_odd")
        halves = {(int(i), p & 1) for p, i in enumerate(idx)}
        assert halves == {(i, h) for i in range(NSET) for h in (0, 1)}       # every filter in both halves
        pairs = {(int(idx[p]), int(idx[p + 1])) for p in range(0, B - 1, 2)}
        assert {(i, (i + 1) % NSET) for i in range(NSET)} <= pairs
    mean, P, st = predict_once(slk, kset, model, per_filter_q, idx)
    np.testing.assert_array_equal(st, ref[2][idx])
    same_bits(mean, ref[0][idx], f"{model} B={B}: mean")
    same_bits(P, ref[1][idx], f"{model} B={B}: P")


def test_status_accumulates_per_half(slk, kset):
    """A second predict ORs into the status words: the failed halves keep SLK_ST_LLT_FAIL, their partners stay clean."""
    B = batch_of(slk, "big_odd")
    idx = np.arange(B) % NSET
    f = slk.Msckf(kset["mean"][idx], kset["P"][idx])
    for _ in range(2):
        f.predict(slk.PM_DELTA_POSE, kset["u"][idx], kset["Q"])
    st = f.status()
    f.close()
    want = np.where((idx == 3) | (idx == 4), slk.ST_LLT_FAIL, 0)
    np.testing.assert_array_equal(st, want)


def test_step_n_beyond_4096_filters_at_k0(slk, kset):
    """k = 0 runs predict in a launch of its own beyond 4096 filters.  Reference: predict, then update, per step, on the set
    alone (the one-wave predict kernel, and the update launch the large batch's step makes after its predict)."""
    T, m = 2, 8
    B = 4096 + 3
    assert B >= slk.PREDICT_PAIR_MIN_BATCH and B % 2 == 1
    good = np.array([0, 1, 2, 5, 6])                            # (the failed filters' updates are not this test's subject)
    s = kset
    rng = np.random.default_rng(0x9A1B0002)
    z = s["z"][good][None] + rng.normal(0, 0.01, (T, good.size, m))
    u = np.broadcast_to(s["u"][good], (T, good.size, 13)).copy()
    feat = np.broadcast_to(s["feat"][good].reshape(good.size, -1), (T, good.size, (m // 2) * 4)).copy()
    parts = []
    for c in chunks(good.size, slk):
        f = slk.Msckf(s["mean"][good][c], s["P"][good][c])
        for t in range(T):
            f.predict(slk.PM_DELTA_POSE, u[t][c], s["Q"])
            f.update(z[t][c], slk.MM_FEATURE_PROJ, feat[t][c], s["R"])
        parts.append((f.muState(), f.getPk(), f.status(), f.outliers()))
        f.close()
    ref = tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
    idx = np.arange(B) % good.size
    g = slk.Msckf(s["mean"][good][idx], s["P"][good][idx])
    g.step_n(slk.PM_DELTA_POSE, np.ascontiguousarray(u[:, idx]), s["Q"], np.ascontiguousarray(z[:, idx]), slk.MM_FEATURE_PROJ,
             np.ascontiguousarray(feat[:, idx]), s["R"])
    mean, P, st, out = g.muState(), g.getPk(), g.status(), g.outliers()
    g.close()
    np.testing.assert_array_equal(st, ref[2][idx])
    np.testing.assert_array_equal(out, ref[3][idx])
    same_bits(mean, ref[0][idx], "step_n k=0: mean")
    same_bits(P, ref[1][idx], "step_n k=0: P")


# ---------------------------------------------------------------- k = 8, m = 8: the benchmark's shape on the smallest pair batch
K8_SET = 5


@pytest.fixture(scope="module")
def k8():
    s = sc.synthetic_msckf(K8_SET, 8, m=8, seed=0x9A1B0008)
    P = s["P"].copy()
    P[1, 3, 3] += 2.0                                            # 1.4 rad in the current state: more passes than its partners
    d = np.ones(s["N"])
    d[3:6] = 1e-3
    P[2] = P[2] * d[:, None] * d[None, :]
    s["P"] = np.ascontiguousarray(P)
    return s


def k8_batches(slk):
    return sorted({slk.PREDICT_PAIR_MIN_BATCH, max(slk.PREDICT_PAIR_MIN_BATCH, 256) + 1})


_K8_REF = {}


def k8_reference(slk, s, what, run):
    """run(filter batch, index block) on batches below the threshold -> (mean, P, status, outliers, records), once per test."""
    if what not in _K8_REF:
        parts = []
        for c in chunks(K8_SET, slk):
            f = slk.Msckf(s["mean"][c], s["P"][c])
            rec = run(f, c)
            parts.append((f.muState(), f.getPk(), f.status(), f.outliers(), rec))
            f.close()
        _K8_REF[what] = tuple(np.concatenate([p[i] for p in parts], axis=(1 if i == 4 else 0)) for i in range(5))
    return _K8_REF[what]


@pytest.mark.parametrize("pos", [0, 1], ids=["smallest", "odd257"])
def test_full_step_k8_on_the_pair_route(slk, k8, pos):
    s, B = k8, k8_batches(slk)[pos]

    def run(f, c):
        f.step(slk.PM_DELTA_POSE, s["u"][c], s["Q"], s["z"][c], slk.MM_FEATURE_PROJ, s["feat"][c], s["R"])
        return np.zeros((1, len(c)))

    ref = k8_reference(slk, s, "step", run)
    assert (ref[2] & ~slk.ST_ALL_REJECTED == 0).all(), ref[2]
    idx = (np.arange(B) + 1) % K8_SET                           # (filters 1 and 2 share the first wave)
    g = slk.Msckf(s["mean"][idx], s["P"][idx])
    run(g, idx)
    mean, P, st, out = g.muState(), g.getPk(), g.status(), g.outliers()
    g.close()
    np.testing.assert_array_equal(st, ref[2][idx])
    np.testing.assert_array_equal(out, ref[3][idx])
    same_bits(mean, ref[0][idx], f"step k=8 B={B}: mean")
    same_bits(P, ref[1][idx], f"step k=8 B={B}: P")


@pytest.mark.parametrize("pos", [0, 1], ids=["smallest", "odd257"])
def test_step_n_two_steps_k8_on_the_pair_route(slk, k8, pos):
    s, B, T, m = k8, k8_batches(slk)[pos], 2, 8
    rng = np.random.default_rng(0x9A1B0009)
    z = s["z"][None] + rng.normal(0, 0.01, (T, K8_SET, m))
    u = np.broadcast_to(s["u"], (T, K8_SET, 13)).copy()
    feat = np.broadcast_to(s["feat"].reshape(K8_SET, -1), (T, K8_SET, (m // 2) * 4)).copy()

    def run(f, c):
        r = f.step_n(slk.PM_DELTA_POSE, np.ascontiguousarray(u[:, c]), s["Q"], np.ascontiguousarray(z[:, c]), slk.MM_FEATURE_PROJ,
                     np.ascontiguousarray(feat[:, c]), s["R"], record_mean=True)
        return r["mean"]

    ref = k8_reference(slk, s, "step_n", run)
    idx = (np.arange(B) + 1) % K8_SET
    g = slk.Msckf(s["mean"][idx], s["P"][idx])
    rec = run(g, idx)
    mean, P, st, out = g.muState(), g.getPk(), g.status(), g.outliers()
    g.close()
    np.testing.assert_array_equal(st, ref[2][idx])
    np.testing.assert_array_equal(out, ref[3][idx])
    for t in range(T):
        same_bits(rec[t], ref[4][t][idx], f"step_n k=8 B={B}: mean record of step {t}")
    same_bits(mean, ref[0][idx], f"step_n k=8 B={B}: mean")
    same_bits(P, ref[1][idx], f"step_n k=8 B={B}: P")


def test_guard_words_behind_an_odd_batch(slk):
    """slk_selftest_predict_pair: both kernels on arrays of its own with guard words behind mean, P and status, an odd batch of
    2049 -- 0 when the guards are intact and the pair kernel's outputs equal the one-wave kernel's word for word."""
    assert slk.load_library().slk_selftest_predict_pair(0) == 0
