"""CPU: the public face of the premultiplied iterations on stored entries
(PFDR_REDUCED_SPARSE_ALL, pfdr_cp_reduce_csc_sparse_preAt_*,
pfdr_cp_solver_premultiplied_stats), and a numpy model of the claim that the
GPU tests stand on: the reduced normal equations summed over the stored
common rows only have the bytes of the sums over every row."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cp_reduced_sparse as RS
import cp_sparse_cases as SC
from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import uniform

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PREAT = ("pfdr_cp_reduce_csc_sparse_preAt_f32", "pfdr_cp_reduce_csc_sparse_preAt_f64")
STATS = "pfdr_cp_solver_premultiplied_stats"
ERR_ARG = 1
F32, F64 = np.float32, np.float64


def test_the_entries_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "pfdr_mi355x.h")).read()
    lib = pfdr.load()
    for name in PREAT + (STATS,):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
    assert STATS in pfdr.EXPORTED and pfdr.EXPORTED_PREAT == PREAT
    assert re.search(r"#define PFDR_REDUCED_SPARSE_ALL 2\b", hdr)
    assert pfdr.PFDR_REDUCED_SPARSE_ALL == 2 == pfdr._reduced_mode("sparse_all")
    assert pfdr._reduced_mode("sparse") == 1 and pfdr._reduced_mode("dense") == 0
    assert lib.pfdr_abi_version() == 4 == pfdr.ABI_VERSION  # functions and a constant only
    assert callable(pfdr.CPSolver.premultiplied_stats)
    assert callable(pfdr.Lib.cp_solver_premultiplied_stats)


def test_python_refuses_before_the_library():
    c = SC.csc("one_row", F32)
    rVc, Vc = SC.partition("bands", c.V)
    Y = np.ones(1, F32)
    with pytest.raises(ValueError, match="CSC"):
        pfdr.cp_reduce(1, c.to_dense(), Y, rVc, Vc, preAt=True, reduced="sparse_all")
    with pytest.raises(ValueError, match="CSC"):
        pfdr.cp_reduce(1, c.to_dense(), Y, rVc, Vc, preAt=False, reduced="sparse_all")
    with pytest.raises(ValueError, match="preAt"):  # as before
        pfdr.cp_reduce(1, c, Y, rVc, Vc, preAt=True, reduced="sparse")
    with pytest.raises(ValueError, match="sparse_all"):
        pfdr._reduced_mode("sparse-all")
    E = np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="CSC"):
        pfdr.CP_quadratic_l1(Y, E, E, np.zeros(0, F32), c.to_dense(), 0.0, reduced="sparse_all")


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_the_step_checks_its_arguments_before_any_device_work(sfx, ct):
    lib = pfdr.load()
    fn = getattr(lib, "pfdr_cp_reduce_csc_sparse_preAt_" + sfx)
    dt = F32 if sfx == "f32" else F64
    c = SC.csc("one_row", dt)
    s = c.struct()
    rVc, Vc = SC.partition("bands", c.V)
    Y = np.ones(1, dt)
    rnnz = C.c_int64(-1)
    colptr, rowidx, val = np.zeros(4, np.int64), np.zeros(c.nnz, np.int32), np.zeros(c.nnz, dt)
    rAA, rY = np.zeros(9, dt), np.zeros(3, dt)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(N=1, csc=C.byref(s), mem=pfdr.PFDR_MEM_HOST, rAA=rAA, rY=rY, out=C.byref(rnnz),
             colptr=colptr, rowidx=rowidx, val=val):
        st = fn(C.c_int(N), C.c_int(c.V), csc, p(Y), C.c_int(3), p(rVc), p(Vc), C.c_int(mem),
                ct(1e-3), C.c_int(100), C.c_int(10), p(rAA), p(rY), None, None, out, p(colptr),
                p(rowidx), p(val))
        return st, lib.pfdr_last_error().decode()

    for kw, needle in ((dict(N=0), "N > 0"), (dict(csc=None), "pfdr_csc is NULL"),
                       (dict(mem=5), "invalid arguments"), (dict(rAA=None), "rAA and rY"),
                       (dict(rY=None), "rAA and rY"), (dict(out=None), "all set or all NULL"),
                       (dict(colptr=None), "all set or all NULL"),
                       (dict(rowidx=None, val=None), "all set or all NULL")):
        st, msg = call(**kw)
        assert st == ERR_ARG and "pfdr_cp_reduce_csc_sparse_preAt_" + sfx in msg and needle in msg, (
            kw, msg)
    assert rnnz.value == -1 and not rAA.any()


def test_the_stats_call_refuses_a_null_handle():
    lib = pfdr.load()
    assert lib.pfdr_cp_solver_premultiplied_stats(None, None, None, None) == ERR_ARG
    assert STATS in lib.pfdr_last_error().decode()


# ------------------------------------------------- the model of the claim --
def _partition(name, V):
    if name == "identity":
        return np.arange(V + 1, dtype=np.int32), np.arange(V, dtype=np.int32)
    return SC.partition(name, V)


CASES = [(m, q) for m in SC.MATRICES for q in SC.PARTITIONS + ("identity",)
         if _partition(q, SC.matrix(m)[0].shape[1]) is not None]


def _seq_all_rows(rA, Y):
    """(rAA, rY): s += a[n] * b[n] for n = 0 .. N - 1 from +0, every pair at
    once (row n's products are rounded, then added: numpy contracts nothing)"""
    rV, N = rA.shape
    G, y = np.zeros((rV, rV), rA.dtype), np.zeros(rV, rA.dtype)
    for n in range(N):
        a = rA[:, n]
        G = G + a[:, None] * a[None, :]
        y = y + a * Y[n]
    return G, y


def _seq_stored_rows(rA, st, Y):
    """the same over the rows stored in both columns (rY: in the column) only;
    elsewhere the sum keeps its bytes"""
    rV, N = rA.shape
    G, y = np.zeros((rV, rV), rA.dtype), np.zeros(rV, rA.dtype)
    for n in range(N):
        a, m = rA[:, n], st[n]
        both = m[:, None] & m[None, :]
        G = np.where(both, G + a[:, None] * a[None, :], G)
        y = np.where(m, y + a * Y[n], y)
    return G, y


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mat,part", CASES, ids=["%s-%s" % c for c in CASES])
def test_the_sums_over_stored_rows_have_the_bytes_of_the_sums_over_all_rows(mat, part, dt):
    c = SC.csc(mat, dt)
    rVc, Vc = _partition(part, c.V)
    rA = SC.model_colsum(c, rVc, Vc)  # (rV, N)
    st = RS.stored_model(c, rVc, Vc)  # (N, rV)
    assert not np.any(rA.T[~st])      # nothing outside the structure
    Y = (2 * uniform(91, np.arange(c.N, dtype=np.uint64)) - 1).astype(dt)
    G0, y0 = _seq_all_rows(rA, Y)
    G1, y1 = _seq_stored_rows(rA, st, Y)
    assert G0.dtype == np.dtype(dt) and np.all(np.isfinite(G0))
    assert SC.same_bytes(G0, G1), np.argwhere(G0 != G1)[:5]
    assert SC.same_bytes(y0, y1), np.flatnonzero(y0 != y1)[:5]
    if mat == "holes":  # the stored zeros and the -0.0 are in the structure
        assert np.any(st & (rA.T == 0))
