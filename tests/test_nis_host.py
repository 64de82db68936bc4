"""CPU-side checks of the innovation-consistency entry points: declared in include/slk.h, exported by the package with
matching argument lists, struct slk_traj and the ABI version unchanged, null handles refused without a device, and the
facade test program compiles against the headers.  No compute calls are made here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("slk_nis", "slk_get_sigma", "slk_step_n_diag")


@pytest.fixture(scope="module")
def slk():
    import __graft_entry__ as ge
    ge.build()
    from slkpkg import slk as mod
    return mod


def header():
    src = open(os.path.join(ROOT, "include", "slk.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_parameters(name):
    """the parameter list of `int name(...)` in the header -> 'p' for a pointer, 'i' for an int"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header())
    assert m, name + " is not declared in include/slk.h"
    kinds = []
    for par in m.group(1).split(","):
        par = par.strip()
        assert par.startswith(("int ", "const ", "double ", "slk_filter ")), par
        kinds.append("p" if "*" in par else "i")
    return "".join(kinds)


def test_new_symbols_are_declared_exported_and_typed(slk):
    lib = slk.load_library()
    for name in NEW:
        assert name in slk.EXPORTS and hasattr(lib, name), name
        fn = getattr(lib, name)
        got = "".join("i" if a is C.c_int else "p" for a in fn.argtypes)
        assert got == declared_parameters(name), (name, got, declared_parameters(name))
        assert all(a is C.c_int or a is C.c_void_p or issubclass(a, C._Pointer) for a in fn.argtypes), name
    assert declared_parameters("slk_nis") == "pipippipippi"
    assert declared_parameters("slk_get_sigma") == "piipi"
    assert declared_parameters("slk_step_n_diag") == "pppipi"


def test_traj_and_abi_version_are_unchanged(slk):
    assert re.search(r"#define\s+SLK_ABI_VERSION\s+1\b", header())
    # struct slk_traj: 26 members, LP64 layout as before the records existed (the new ones live in slk_traj_diag)
    assert len(slk.Traj._fields_) == 26 and C.sizeof(slk.Traj) == 192
    assert [n for n, _ in slk.TrajDiag._fields_] == ["nis_hist", "logdet_hist", "sigma_hist"]
    assert C.sizeof(slk.TrajDiag) == 3 * C.sizeof(C.c_void_p)
    m = re.search(r"typedef\s+struct\s+slk_traj_diag\s*\{(.*?)\}\s*slk_traj_diag\s*;", header(), flags=re.S)
    assert m and re.findall(r"double\s*\*\s*(\w+)\s*;", m.group(1)) == ["nis_hist", "logdet_hist", "sigma_hist"]


def test_null_handles_are_refused_without_a_device(slk):
    lib = slk.load_library()
    buf = (C.c_double * 4)()
    p = C.addressof(buf)
    assert lib.slk_nis(None, 2, p, 0, None, p, 2, p, 0, p, None, slk.HOST) == slk.E_INVALID
    assert lib.slk_get_sigma(None, 0, 1, p, slk.HOST) == slk.E_INVALID
    assert lib.slk_step_n_diag(None, None, None, 0, None, slk.HOST) == slk.E_INVALID


def test_step_n_rejects_unknown_records(slk):
    f = slk._FilterBatch.__new__(slk.Msckf)          # (no handle: the argument check comes first)
    f._h = None
    import numpy as np
    with pytest.raises(slk.SlkError, match="diag"):
        slk._FilterBatch.step_n(f, 2, np.zeros((1, 1, 13)), np.eye(12), np.zeros((1, 1, 2)), 2, np.zeros((1, 1, 4)), np.eye(2),
                                diag=("nees",))


def test_nis_facade_program_compiles(slk):
    import facade_build
    exe = facade_build.build("nis_facade")
    assert os.path.exists(exe)
