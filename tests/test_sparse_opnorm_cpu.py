"""Operator norm and diagonal Lipschitz metric of a sparse A (CSC), what holds
without a GPU: the four entries exist, their argument errors come before any
device work, and valid arguments fail loudly where there is no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cp_pfdr_graph_d1_amd import pfdr

NEW = ("pfdr_operator_norm_csc_f32", "pfdr_operator_norm_csc_f64",
       "pfdr_lipschitz_diag_csc_f32", "pfdr_lipschitz_diag_csc_f64")
ERR_ARG = 1
DTS = [("f32", np.float32), ("f64", np.float64)]


def test_the_four_entries_are_declared_exported_and_loaded():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pfdr_mi355x.h")) as f:
        header = f.read()
    lib = pfdr.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pfdr.EXPORTED, name
        assert hasattr(lib, name), name
    assert re.search(r"int\s+pfdr_abi_version\(void\);\s*/\*\s*4\b", header)  # additive
    assert lib.pfdr_abi_version() == 4 == pfdr.ABI_VERSION
    assert callable(pfdr.lipschitz_diag)


def _csc(dt, N=3, V=4, **over):
    """a well-formed 3-by-4 CSC, one entry per column -> (N, V, CSCStruct, the
    arrays to keep alive)"""
    colptr = np.arange(5, dtype=np.int64)
    rowidx = (np.arange(4) % 3).astype(np.int32)
    val = np.ones(4, dt)
    s = pfdr.CSCStruct(4, colptr.ctypes.data, rowidx.ctypes.data, val.ctypes.data)
    for k, v in over.items():
        setattr(s, k, v)
    return N, V, s, (colptr, rowidx, val)


def _norm(sfx, dt, N, V, s, mem=0, itMax=10, out=True):
    lib = pfdr.load()
    ct = C.c_float if dt == np.float32 else C.c_double
    res = ct(-1.0)
    st = getattr(lib, "pfdr_operator_norm_csc_" + sfx)(
        N, V, None if s is None else C.byref(s), mem, ct(1e-3), itMax, 10, 0,
        C.byref(res) if out else None, None)
    return st, lib.pfdr_last_error().decode(), res.value


def _diag(sfx, dt, N, V, s, mem=0, out=True):
    lib = pfdr.load()
    L = np.full(max(V, 1), -1.0, dt)
    st = getattr(lib, "pfdr_lipschitz_diag_csc_" + sfx)(
        N, V, None if s is None else C.byref(s), mem, L.ctypes.data if out else None, None)
    return st, lib.pfdr_last_error().decode(), L


REFUSED = [
    ("N_zero", dict(N=0), {}, "N > 0"),
    ("N_negative", dict(N=-3), {}, "N > 0"),
    ("V_zero", dict(V=0), {}, "V > 0"),
    ("V_negative", dict(V=-4), {}, "V > 0"),
    ("mem", dict(mem=7), {}, "mem"),
    ("null_csc", dict(null=True), {}, "NULL"),
    ("null_colptr", {}, dict(colptr=None), "NULL array"),
    ("null_rowidx", {}, dict(rowidx=None), "NULL array"),
    ("null_val", {}, dict(val=None), "NULL array"),
    ("nnz_zero", {}, dict(nnz=0), "nnz"),
    ("nnz_negative", {}, dict(nnz=-1), "nnz"),
    ("nnz_huge", {}, dict(nnz=2 ** 31 - 256), "nnz"),
    ("null_output", dict(out=False), {}, "is NULL"),
]


@pytest.mark.parametrize("sfx,dt", DTS)
@pytest.mark.parametrize("entry", ["norm", "diag"])
@pytest.mark.parametrize("name,args,over,needle", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_before_any_device_work(entry, sfx, dt, name, args, over, needle):
    """Where there is no GPU, PFDR_ERR_ARG (not PFDR_ERR_HIP) with its message
    shows that the check precedes the first device call."""
    args = dict(args)
    N, V, s, keep = _csc(dt, **over)
    N, V = args.pop("N", N), args.pop("V", V)
    if args.pop("null", False):
        s = None
    fn = _norm if entry == "norm" else _diag
    st, msg, _ = fn(sfx, dt, N, V, s, **args)
    assert st == ERR_ARG, (st, msg)
    which = "pfdr_operator_norm_csc_" if entry == "norm" else "pfdr_lipschitz_diag_csc_"
    assert which + sfx in msg and needle in msg, msg


@pytest.mark.parametrize("sfx,dt", DTS)
def test_python_mirrors_raise_naming_the_offence(sfx, dt):
    one = pfdr.CSC(np.arange(5), np.arange(4) % 3, np.ones(4, dt), 0)
    with pytest.raises(pfdr.PFDRError, match="N > 0"):
        pfdr.operator_norm(one)
    with pytest.raises(pfdr.PFDRError, match="N > 0"):
        pfdr.lipschitz_diag(one)
    empty = pfdr.CSC(np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, dt), 3)
    with pytest.raises(pfdr.PFDRError, match="nnz"):
        pfdr.operator_norm(empty)
    with pytest.raises(pfdr.PFDRError, match="nnz"):
        pfdr.lipschitz_diag(empty)
    with pytest.raises(TypeError):
        pfdr.lipschitz_diag(np.ones((3, 4), dt))


@pytest.mark.parametrize("sfx,dt", DTS)
def test_negative_itmax_is_the_dense_entrys_business(sfx, dt):
    """The dense entry takes a negative itMax (no iteration after the first
    product), so the sparse one does not refuse it: without a device the call
    gets as far as the device and fails there, not on its arguments."""
    if pfdr.load().pfdr_device_count() >= 1:
        pytest.skip("a GPU is visible: tests/test_sparse_opnorm_gpu.py runs this call")
    N, V, s, keep = _csc(dt)
    st, msg, _ = _norm(sfx, dt, N, V, s, itMax=-1)
    assert st != 0 and st != ERR_ARG, (st, msg)


@pytest.mark.parametrize("sfx,dt", DTS)
def test_valid_arguments_fail_loudly_without_a_gpu(sfx, dt):
    if pfdr.load().pfdr_device_count() >= 1:
        pytest.skip("a GPU is visible: tests/test_sparse_opnorm_gpu.py runs these calls")
    N, V, s, keep = _csc(dt)
    st, msg, val = _norm(sfx, dt, N, V, s)
    assert st != 0 and "pfdr_operator_norm_csc_" + sfx in msg, (st, msg)
    st, msg, L = _diag(sfx, dt, N, V, s)
    assert st != 0 and "pfdr_lipschitz_diag_csc_" + sfx in msg, (st, msg)
    one = pfdr.CSC(keep[0], keep[1], keep[2], 3)
    with pytest.raises(pfdr.PFDRError):
        pfdr.operator_norm(one)
    with pytest.raises(pfdr.PFDRError):
        pfdr.lipschitz_diag(one)


def test_front_end_refuses_an_unknown_lipschitz_choice_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(pfdr, "load", no_library)
    monkeypatch.setattr(pfdr, "Lib", no_library)
    csc = pfdr.CSC(np.arange(5), np.arange(4) % 3, np.ones(4, np.float32), 3)
    z = np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="lipschitz"):
        pfdr.PFDR_quadratic_l1(np.ones(3, np.float32), z, z, 0.1, csc, 0.01,
                               lipschitz="nonsense")
