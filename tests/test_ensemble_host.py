"""CPU-side checks of the ensemble calls (slk_ensemble_moments / slk_gather_states): the numpy twin of
tests/ensemble_ref.py against numpy's own weighted statistics where the manifold is flat, the fixed point of its pinned
iteration, the number of passes it makes on every input set the GPU tests use (fewer than 20: what keeps their centre
tolerance meaningful), and the two symbols declared, exported, typed and refusing a null handle without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as o
import ensemble_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("slk_ensemble_moments", "slk_gather_states")
VECTOR_RANGES = [(0, 3), (6, 6), (7, 1)]                # position; velocity and angular velocity; one component


@pytest.fixture(scope="module")
def slk():
    import __graft_entry__ as ge
    ge.build()
    from slkpkg import slk as mod
    return mod


def rel_close(a, b, rel=1e-12):
    scale = np.abs(b).max()
    assert np.abs(a - b).max() <= rel * scale, (np.abs(a - b).max(), scale)


# ------------------------------------------------------------------ 1. the twin against numpy where the manifold is flat
@pytest.mark.parametrize("wkind", ["uniform", "random"])
@pytest.mark.parametrize("groups", [1, 4])
def test_twin_equals_numpy_on_vector_ranges(wkind, groups):
    b = er.bank("msckf_n12", groups)
    B, Bg, lay = b["B"], b["B"] // groups, b["lay"]
    w = er.weights_of(wkind, B, groups)
    truth = er.truth_of(b)
    wv = np.ones(B) if w is None else w
    te, tm = er.Twin(lay, b["mean"], w, truth, groups), er.Twin(lay, b["mean"], w, None, groups)
    storage = {0: 0, 6: 7, 7: 8}                        # tangent -> storage offset of these vector ranges (Msckf)
    for t0, n in VECTOR_RANGES:
        me, mm = te.moments(b["P"], t0, n), tm.moments(b["P"], t0, n)
        s0 = storage[t0]
        for g in range(groups):
            sl = slice(g * Bg, (g + 1) * Bg)
            e = truth[sl, s0:s0 + n] - b["mean"][sl, s0:s0 + n]
            mu = b["mean"][sl, s0:s0 + n]
            rel_close(me["center"][g], np.average(e, axis=0, weights=wv[sl]))
            rel_close(me["spread"][g], np.cov(e.T, aweights=wv[sl], ddof=0).reshape(n, n))
            rel_close(mm["center"][g, s0:s0 + n], np.average(mu, axis=0, weights=wv[sl]))
            rel_close(mm["spread"][g], np.cov(mu.T, aweights=wv[sl], ddof=0).reshape(n, n))
            rel_close(me["mean_cov"][g], np.average(b["P"][sl, t0:t0 + n, t0:t0 + n], axis=0, weights=wv[sl]))
            assert me["mean_cov"][g].tobytes() == mm["mean_cov"][g].tobytes()
            rel_close(me["ess"][g:g + 1], np.array([wv[sl].sum() ** 2 / (wv[sl] ** 2).sum()]))


# ------------------------------------------------------------------ 2. the centre is a fixed point; 3. in < 20 passes
@pytest.mark.parametrize("name", er.SHAPE_IDS)
def test_centre_is_a_fixed_point_reached_in_few_passes(name):
    """every (shape, G, weights) the GPU tests run in mixture mode"""
    B = er.SHAPES[er.SHAPE_IDS.index(name)][3]
    for groups in er.group_counts(B):
        b = er.bank(name, groups)
        lay, Bg = b["lay"], B // groups
        # the inputs keep the promise the iteration count rests on: rotations within ROT_SPREAD of the group's first
        for t in er.so3_toffs(lay):
            d = np.stack([o.boxminus(lay, b["mean"][i], b["mean"][i // Bg * Bg])[t:t + 3] for i in range(0, B, 7)])
            assert np.linalg.norm(d, axis=1).max() <= er.ROT_SPREAD / 2 + 1e-9
        for wkind in er.WEIGHT_KINDS:
            tw = er.Twin(lay, b["mean"], er.weights_of(wkind, B, groups), None, groups)
            good = np.flatnonzero(~tw.bad)
            assert good.size, (name, groups, wkind)
            assert tw.passes[good].max() < 20, (name, groups, wkind, tw.passes.max())
            for g in good[:: max(1, good.size // 4)]:
                sl = slice(g * Bg, (g + 1) * Bg)
                r = sum(tw.wn[i] * o.boxminus(lay, b["mean"][i], tw.centre[g]) for i in range(sl.start, sl.stop))
                assert np.linalg.norm(r) <= 1e-11, (name, groups, wkind, g, np.linalg.norm(r))


@pytest.mark.parametrize("name", ["msckf_n60", "usckf_n48"])
def test_step_inputs_of_the_lower_only_tests(name):
    """the banks the GPU tests step before they take moments: as tight as the others"""
    b, s = er.step_inputs(name, 4, 64)
    assert s["mean"] is b["mean"] and s["z"].shape[0] == 64
    tw = er.Twin(b["lay"], b["mean"], None, None, 4)
    assert tw.passes.max() < 20


def test_twin_nan_convention_and_gather():
    b = er.bank("msckf_n12", 8)
    B, lay = b["B"], b["lay"]
    w = np.random.default_rng(1).uniform(0.5, 1.0, B)
    Bg = B // 8
    w[2 * Bg:3 * Bg] = 0.0
    w[5 * Bg + 3] = np.nan
    w[6 * Bg + 1] = -1.0
    w[7 * Bg] = np.inf
    m = er.moments(lay, b["mean"], b["P"], w, None, 0, 6, 8)
    for g in range(8):
        bad = g in (2, 5, 6, 7)
        for name in ("center", "spread", "mean_cov", "ess"):
            assert np.isnan(m[name][g]).all() == bad and np.isnan(m[name][g]).any() == bad, (g, name)
    src = np.random.default_rng(2).integers(0, B, B)
    st, oc = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.uint32)[::-1].copy()
    gm, gP, gs, go = er.gather(b["mean"], b["P"], st, oc, src)
    assert (gm[5] == b["mean"][src[5]]).all() and (gP[9] == b["P"][src[9]]).all() and gs[3] == st[src[3]] and go[4] == oc[src[4]]


# ------------------------------------------------------------------ 4. the ABI
def header():
    src = open(os.path.join(ROOT, "include", "slk.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_parameters(name):
    """the parameter list of `int name(...)` in the header -> 'p' for a pointer, 'i' for an int"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header())
    assert m, name + " is not declared in include/slk.h"
    return "".join("p" if "*" in par else "i" for par in m.group(1).split(","))


def test_symbols_are_declared_exported_and_typed(slk):
    lib = slk.load_library()
    for name in NEW:
        assert name in slk.EXPORTS and hasattr(lib, name), name
        got = "".join("i" if a is C.c_int else "p" for a in getattr(lib, name).argtypes)
        assert got == declared_parameters(name), (name, got, declared_parameters(name))
    assert declared_parameters("slk_ensemble_moments") == "pippiippppi"
    assert declared_parameters("slk_gather_states") == "ppi"
    assert re.search(r"#define\s+SLK_ABI_VERSION\s+1\b", header())
    assert C.sizeof(slk.Traj) == 192 and C.sizeof(slk.TrajDiag) == 3 * C.sizeof(C.c_void_p)     # the frozen structs
    assert hasattr(slk._FilterBatch, "ensemble_moments") and hasattr(slk._FilterBatch, "gather")


def test_null_handles_are_refused_without_a_device(slk):
    lib = slk.load_library()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    assert lib.slk_ensemble_moments(None, 1, None, None, 0, 1, p, p, p, p, slk.HOST) == slk.E_INVALID
    assert lib.slk_ensemble_moments(None, 1, p, p, 0, 1, p, None, None, None, slk.DEVICE) == slk.E_INVALID
    assert lib.slk_gather_states(None, p, slk.HOST) == slk.E_INVALID
    assert lib.slk_gather_states(None, None, slk.DEVICE) == slk.E_INVALID


def test_ensemble_facade_program_compiles(slk):
    import facade_build
    exe = facade_build.build("ensemble_facade")
    assert os.path.exists(exe)
