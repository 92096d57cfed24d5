"""Sparse A (CSC) in cut pursuit, what holds without a GPU: the four entries
exist, their argument errors come before any device work, and the sums the
GPU tests compare are sensitive to the order the issue fixes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cp_sparse_cases as SC
from cp_pfdr_graph_d1_amd import pfdr

NEW = ("pfdr_cp_reduce_csc_f32", "pfdr_cp_reduce_csc_f64", "pfdr_cpgraph_gradient_csc",
       "pfdr_cp_solver_create_sparse")
ERR_ARG = 1


def test_the_four_entries_are_declared_exported_and_loaded():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pfdr_mi355x.h")) as f:
        header = f.read()
    lib = pfdr.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pfdr.EXPORTED, name
        assert hasattr(lib, name), name
    assert lib.pfdr_abi_version() == 4 == pfdr.ABI_VERSION
    assert "keep their dense A" not in header


def _problem(kind=pfdr.PFDR_KIND_L1, N=3, V=4, dt=np.float32, **over):
    """a well-formed problem and CSC (3-by-4, one entry per column); -> (CPProblem,
    CSCStruct, the arrays to keep alive)"""
    Y = np.ones(max(N, V), dt)
    colptr = np.arange(V + 1, dtype=np.int64)
    rowidx = (np.arange(V) % 3).astype(np.int32)
    val = np.ones(V, dt)
    p = pfdr.CPProblem()
    p.kind, p.dtype, p.mem = kind, pfdr.PFDR_F32 if dt == np.float32 else pfdr.PFDR_F64, 0
    p.V, p.E, p.N, p.K = V, 0, N, 3 if kind == pfdr.PFDR_KIND_SIMPLEX else 0
    p.Y = Y.ctypes.data
    p.min, p.max = -1.0, 1.0
    s = pfdr.CSCStruct(V, colptr.ctypes.data, rowidx.ctypes.data, val.ctypes.data)
    for k, v in over.items():
        setattr(s if k in ("nnz", "colptr", "rowidx", "val") else p, k, v)
    return p, s, (Y, colptr, rowidx, val)


REFUSED = [
    ("simplex", dict(kind=pfdr.PFDR_KIND_SIMPLEX, N=0), "simplex"),
    ("N_zero", dict(N=0), "N > 0"),
    ("N_negative", dict(N=-4), "N > 0"),
    ("dense_A_too", dict(A="Y"), "both"),
    ("null_csc", dict(csc=None), "NULL"),
    ("null_colptr", dict(colptr=None), "NULL array"),
    ("null_rowidx", dict(rowidx=None), "NULL array"),
    ("null_val", dict(val=None), "NULL array"),
    ("nnz_zero", dict(nnz=0), "nnz"),
    ("nnz_huge", dict(nnz=2 ** 31 - 256), "nnz"),
]


@pytest.mark.parametrize("kind", [pfdr.PFDR_KIND_L1, pfdr.PFDR_KIND_BOUNDS], ids=["l1", "bounds"])
@pytest.mark.parametrize("name,over,needle", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_sparse_refuses_before_any_device_work(kind, name, over, needle):
    """Where there is no GPU, PFDR_ERR_ARG (not PFDR_ERR_HIP) with its message
    shows that the check precedes the first device call."""
    over = dict(over)
    over.setdefault("kind", kind)
    null_csc = "csc" in over and over.pop("csc") is None
    dense_too = over.pop("A", None)
    p, s, keep = _problem(**over)
    if dense_too:
        p.A = keep[0].ctypes.data
    lib = pfdr.load()
    h = C.c_void_p(12345)
    st = lib.pfdr_cp_solver_create_sparse(C.byref(h), C.byref(p), None if null_csc else C.byref(s))
    msg = lib.pfdr_last_error().decode()
    assert st == ERR_ARG, (st, msg)
    assert "pfdr_cp_solver_create_sparse" in msg and needle in msg, msg
    assert h.value is None  # no handle


@pytest.mark.parametrize("sfx,dt", [("f32", np.float32), ("f64", np.float64)])
@pytest.mark.parametrize("N", [0, -4])
def test_reduce_csc_needs_a_positive_N(sfx, dt, N):
    p, s, keep = _problem(dt=dt)
    lib = pfdr.load()
    out = np.zeros(16, dt)
    ptr = np.array([0, 4], np.int32)
    Vc = np.arange(4, dtype=np.int32)
    ct = C.c_float if dt == np.float32 else C.c_double
    vp = lambda a: C.c_void_p(a.ctypes.data)
    st = getattr(lib, "pfdr_cp_reduce_csc_" + sfx)(
        C.c_int(N), C.c_int(4), C.byref(s), vp(keep[0]), C.c_int(1), vp(ptr), vp(Vc), C.c_int(1),
        C.c_int(0), ct(1e-3), C.c_int(100), C.c_int(10), vp(out), vp(out), vp(out), vp(out), None)
    msg = lib.pfdr_last_error().decode()
    assert st == ERR_ARG and "pfdr_cp_reduce_csc_" + sfx in msg and "N > 0" in msg, (st, msg)


def test_the_python_front_ends_refuse_a_mismatched_csc_without_a_device():
    c = SC.csc("one_row", np.float32)
    z = np.zeros(0, np.int32)
    with pytest.raises(pfdr.PFDRError, match="simplex"):
        pfdr.CPSolver("simplex", np.ones(12, np.float32), z, z, np.zeros(0, np.float32), A=c, K=3)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_sums_depend_on_the_list_order(dt):
    """The precondition of the GPU test's power: for r300 under one_perm the
    sequential sums in Vc order differ from those in ascending column order, so
    an implementation that adds in column order cannot give the dense entry's
    bytes; and leaving the dense zeros out changes no sum."""
    c = SC.csc("r300", dt)
    rVc, Vc = SC.partition("one_perm", c.V)
    in_list = SC.model_colsum(c, rVc, Vc)
    in_column = SC.model_colsum(c, rVc, Vc, order="column")
    differ = int((in_list != in_column).any(axis=0).sum())
    dense = SC.model_colsum_dense(SC.matrix("r300")[0].astype(dt), rVc, Vc)
    print(np.dtype(dt).name, "rows whose sum depends on the order:", differ, "of", c.N)
    assert differ >= 1
    assert SC.same_bytes(in_list, dense)


def test_the_model_starts_from_plus_zero():
    """holes: the stored -0.0 is alone in its (row, component) pair under the
    singletons, where the dense loop gives +0.0"""
    c = SC.csc("holes", np.float32)
    r, v = SC.HOLES_NEG_ZERO
    assert np.signbit(c.to_dense()[r, v])
    rVc, Vc = SC.partition("singletons", c.V)
    rA = SC.model_colsum(c, rVc, Vc)
    assert not np.signbit(rA[SC.cv_of(rVc, Vc)[v], r])
    for row in SC.HOLES_EMPTY_ROWS:
        assert not rA[:, row].any()
    assert SC.same_bytes(rA, SC.model_colsum_dense(SC.matrix("holes")[0].astype(np.float32),
                                                   rVc, Vc))


def test_cases_are_what_the_issue_names():
    for name, shape in (("r300", (200, 300)), ("blur", (480, 480)), ("one_row", (1, 12)),
                        ("holes", (200, 300)), ("longrun", (40, 1200))):
        A, st = SC.matrix(name)
        assert A.shape == shape and st.any(axis=0).all(), name
        for part in SC.PARTITIONS:
            pv = SC.partition(part, shape[1])
            if pv is None:
                assert part == "mixed" and shape[1] < 453
                continue
            rVc, Vc = pv
            assert rVc[0] == 0 and rVc[-1] == shape[1] and (np.diff(rVc) > 0).all()
            assert np.array_equal(np.sort(Vc), np.arange(shape[1]))
    A, st = SC.matrix("longrun")
    assert st[3, :1000].all() and (A[3, :1000] != 0).all()
    A, st = SC.matrix("holes")
    assert st[:, 20].all() and st[:, 10].sum() == 1
    others = ~np.isin(np.arange(300), (20, SC.HOLES_NEG_ZERO[1]))
    assert not st[list(SC.HOLES_EMPTY_ROWS)][:, others].any()
    assert not A[list(SC.HOLES_EMPTY_ROWS)].any()  # what is stored there is +-0
    A, _ = SC.matrix("blur")
    assert np.allclose(A.sum(axis=1), 1.0) and (A != 0).sum(axis=1).max() == 9
