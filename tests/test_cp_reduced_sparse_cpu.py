"""CPU: the public face of the sparse reduced operator -- the header, the
Python mirrors, and the argument errors that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cp_sparse_cases as SC
from cp_pfdr_graph_d1_amd import pfdr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("pfdr_cp_reduce_csc_sparse_f32", "pfdr_cp_reduce_csc_sparse_f64",
       "pfdr_cp_solver_set_reduced", "pfdr_cp_solver_reduced_stats")
ERR_ARG = 1


def test_the_entries_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "pfdr_mi355x.h")).read()
    lib = pfdr.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pfdr.EXPORTED and hasattr(lib, name), name
    for name, value in (("PFDR_REDUCED_DENSE", 0), ("PFDR_REDUCED_SPARSE", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
        assert getattr(pfdr, name) == value
    assert lib.pfdr_abi_version() == 4  # functions only: no struct changed


def test_python_face():
    for n in ("set_reduced", "reduced_stats"):
        assert callable(getattr(pfdr.Lib, "cp_solver_" + n)), n
        assert callable(getattr(pfdr.CPSolver, n)), n
    assert inspect.signature(pfdr.cp_reduce).parameters["reduced"].default == "dense"
    for fn in (pfdr.CP_quadratic_l1, pfdr.CP_quadratic_l1_duplex,
               pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex, pfdr.CP_PFDR_graph_quadratic_d1_bounds):
        assert inspect.signature(fn).parameters["reduced"].default == "dense", fn.__name__


def test_python_refuses_before_the_library():
    c = SC.csc("one_row", np.float32)
    rVc, Vc = SC.partition("bands", c.V)
    Y = np.ones(1, np.float32)
    with pytest.raises(ValueError, match="preAt"):
        pfdr.cp_reduce(1, c, Y, rVc, Vc, preAt=True, reduced="sparse")
    with pytest.raises(ValueError, match="CSC"):
        pfdr.cp_reduce(1, c.to_dense(), Y, rVc, Vc, preAt=False, reduced="sparse")
    with pytest.raises(ValueError, match="dense.*sparse"):
        pfdr.cp_reduce(1, c, Y, rVc, Vc, preAt=False, reduced="csr")
    E = np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="CSC"):
        pfdr.CP_quadratic_l1(Y, E, E, np.zeros(0, np.float32), c.to_dense(), 0.0,
                             reduced="sparse")
    with pytest.raises(ValueError, match="dense.*sparse"):
        pfdr.CPSolver("l1", Y, E, E, np.zeros(0, np.float32), A=c, reduced="csr")


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_the_step_checks_its_arguments_before_any_device_work(sfx, ct):
    lib = pfdr.load()
    fn = getattr(lib, "pfdr_cp_reduce_csc_sparse_" + sfx)
    dt = np.float32 if sfx == "f32" else np.float64
    c = SC.csc("one_row", dt)
    s = c.struct()
    rVc, Vc = SC.partition("bands", c.V)
    Y = np.ones(1, dt)
    rnnz = C.c_int64(-1)
    colptr, rowidx, val = np.zeros(4, np.int64), np.zeros(c.nnz, np.int32), np.zeros(c.nnz, dt)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(N=1, csc=C.byref(s), out=C.byref(rnnz), mem=pfdr.PFDR_MEM_HOST):
        st = fn(C.c_int(N), C.c_int(c.V), csc, p(Y), C.c_int(3), p(rVc), p(Vc), C.c_int(mem),
                ct(1e-3), C.c_int(100), C.c_int(10), out, p(colptr), p(rowidx), p(val), None,
                None)
        return st, lib.pfdr_last_error().decode()

    for kw, needle in ((dict(N=0), "N > 0"), (dict(csc=None), "pfdr_csc is NULL"),
                       (dict(out=None), "rnnz"), (dict(mem=5), "invalid arguments")):
        st, msg = call(**kw)
        assert st == ERR_ARG and "pfdr_cp_reduce_csc_sparse_" + sfx in msg and needle in msg, msg
    assert rnnz.value == -1


def test_the_solver_calls_refuse_a_null_handle():
    lib = pfdr.load()
    assert lib.pfdr_cp_solver_set_reduced(None, 1) == ERR_ARG
    assert "pfdr_cp_solver_set_reduced" in lib.pfdr_last_error().decode()
    assert lib.pfdr_cp_solver_reduced_stats(None, None, None, None) == ERR_ARG
