"""GPU: every entry that takes a pfdr_csc refuses a malformed one in the same
words.

One small matrix (6-by-5, f32, an empty row, a column of three entries), four
defects of its colptr / rowidx, seven entries.  Each entry returns
PFDR_ERR_ARG, and the message after the entry's own "name: " prefix is the
same text whichever entry speaks; the well-formed matrix is then accepted by
every one of them.
"""
import ctypes as C

import numpy as np
import pytest

from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

F32 = np.float32
N, V = 6, 5
#           column 0        1       2       3      4      (row 4 holds no entry)
COLPTR = np.array([0, 3, 5, 7, 9, 10], np.int64)
ROWIDX = np.array([0, 1, 3, 1, 2, 0, 5, 2, 3, 5], np.int32)
VAL = np.array([1.0, -0.5, 0.25, 2.0, 0.75, -1.5, 0.5, 1.25, -0.75, 1.0], F32)
NNZ = int(ROWIDX.size)

DEFECTS = ["colptr0", "colptr_end", "row_is_N", "row_repeated"]


def _arrays(defect):
    cp, ri = COLPTR.copy(), ROWIDX.copy()
    if defect == "colptr0":
        cp[0] = 1
    elif defect == "colptr_end":
        cp[V] = NNZ - 1
    elif defect == "row_is_N":
        ri[2] = N  # column 0: rows 0, 1, N
    elif defect == "row_repeated":
        ri[1] = ri[0]  # column 0: rows 0, 0, 3
    else:
        assert defect is None
    return cp, ri, VAL.copy()


def _p(a):
    return C.c_void_p(a.ctypes.data)


# the graph and the values beside A: a chain on the V vertices, two components
EU, EV = np.arange(V - 1, dtype=np.int32), np.arange(1, V, dtype=np.int32)
LA = np.full(V - 1, 0.1, F32)
Y = np.array([0.5, -1.0, 0.25, 1.5, 0.0, -0.75], F32)
RVC = np.array([0, 2, 5], np.int32)
VC = np.arange(V, dtype=np.int32)
RV = 2
BOUND = np.array([40.0], F32)  # above ||A||_1 ||A||_inf = 3.25 * 3.75 >= ||A||^2


def _session(lib, S):
    X0 = np.zeros(V, F32)
    P = pfdr.Problem()
    P.kind, P.dtype, P.mem = pfdr.PFDR_KIND_L1, pfdr.PFDR_F32, pfdr.PFDR_MEM_HOST
    P.V, P.E, P.N = V, V - 1, N
    P.X, P.Y, P.Eu, P.Ev, P.La_d1 = _p(X0), _p(Y), _p(EU), _p(EV), _p(LA)
    P.L, P.Ltype = _p(BOUND), pfdr.SCAL
    P.min, P.max = -np.inf, np.inf
    P.rho, P.condMin, P.itMax = 1.5, 1e-3, 5
    h = C.c_void_p()
    st = lib.pfdr_session_create_sparse(C.byref(h), C.byref(P), C.byref(S))
    if st == 0:
        lib.pfdr_session_destroy(h)
    return st


def _opnorm(lib, S):
    out, ms = C.c_float(0), (C.c_double * 2)()
    return lib.pfdr_operator_norm_csc_f32(N, V, C.byref(S), pfdr.PFDR_MEM_HOST, C.c_float(1e-3),
                                          20, 2, 0, C.byref(out), ms)


def _lipschitz(lib, S):
    L, bound = np.zeros(V, F32), C.c_float(0)
    return lib.pfdr_lipschitz_diag_csc_f32(N, V, C.byref(S), pfdr.PFDR_MEM_HOST, _p(L),
                                           C.byref(bound))


def _reduce(lib, S):
    rA, L, Leq = np.zeros((RV, N), F32), np.zeros(RV, F32), np.zeros(RV, F32)
    return lib.pfdr_cp_reduce_csc_f32(
        C.c_int(N), C.c_int(V), C.byref(S), _p(Y), C.c_int(RV), _p(RVC), _p(VC), C.c_int(0),
        pfdr.PFDR_MEM_HOST, C.c_float(1e-3), C.c_int(20), C.c_int(2), _p(rA), None, None, _p(L),
        _p(Leq))


def _reduce_sparse(lib, S):
    rnnz, rcolptr = C.c_int64(0), np.zeros(RV + 1, np.int64)
    rrowidx, rval = np.zeros(NNZ, np.int32), np.zeros(NNZ, F32)
    L, Leq = np.zeros(RV, F32), np.zeros(RV, F32)
    return lib.pfdr_cp_reduce_csc_sparse_f32(
        C.c_int(N), C.c_int(V), C.byref(S), _p(Y), C.c_int(RV), _p(RVC), _p(VC),
        pfdr.PFDR_MEM_HOST, C.c_float(1e-3), C.c_int(20), C.c_int(2), C.byref(rnnz), _p(rcolptr),
        _p(rrowidx), _p(rval), _p(L), _p(Leq))


def _gradient(lib, S):
    g = pfdr.CPGraph(V, EU, EV, LA)
    try:
        g.set_components(np.repeat(np.arange(RV, dtype=np.int32), np.diff(RVC)), VC, RVC)
        g.set_values(np.array([0.5, -0.25], F32))
        DfS = np.zeros(V, F32)
        return lib.pfdr_cpgraph_gradient_csc(g.h, C.c_int(N), C.byref(S), _p(Y),
                                             pfdr.PFDR_MEM_HOST, _p(DfS))
    finally:
        g.close()


def _solver(lib, S):
    q = pfdr.CPProblem()
    q.kind, q.dtype, q.mem = pfdr.PFDR_KIND_L1, pfdr.PFDR_F32, pfdr.PFDR_MEM_HOST
    q.V, q.E, q.N = V, V - 1, N
    q.Y, q.Eu, q.Ev, q.La_d1 = _p(Y), _p(EU), _p(EV), _p(LA)
    h = C.c_void_p()
    st = lib.pfdr_cp_solver_create_sparse(C.byref(h), C.byref(q), C.byref(S))
    if st == 0:
        lib.pfdr_cp_solver_destroy(h)
    return st


ENTRIES = [("pfdr_session_create_sparse", _session),
           ("pfdr_operator_norm_csc_f32", _opnorm),
           ("pfdr_lipschitz_diag_csc_f32", _lipschitz),
           ("pfdr_cp_reduce_csc_f32", _reduce),
           ("pfdr_cp_reduce_csc_sparse_f32", _reduce_sparse),
           ("pfdr_cpgraph_gradient_csc", _gradient),
           ("pfdr_cp_solver_create_sparse", _solver)]


def _call(lib, fn, defect):
    """-> (status, the message after the entry's "name: " prefix)"""
    cp, ri, va = _arrays(defect)
    S = pfdr.CSCStruct(NNZ, cp.ctypes.data, ri.ctypes.data, va.ctypes.data)
    name, call = fn
    st = call(lib, S)
    msg = lib.pfdr_last_error().decode() if st else ""
    if st:
        assert msg.startswith(name + ": "), (name, msg)
        msg = msg[len(name) + 2:]
    return st, msg


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_entry_refuses_a_malformed_csc_in_the_same_words(gpu_lib, defect):
    lib = pfdr.load()
    said = {}
    for fn in ENTRIES:
        st, msg = _call(lib, fn, defect)
        print(defect, fn[0], st, repr(msg))
        assert st == 1, (defect, fn[0], st, msg)  # PFDR_ERR_ARG
        said[fn[0]] = msg
    first = said[ENTRIES[0][0]]
    assert first.startswith("sparse A: "), first
    assert all(m == first for m in said.values()), (defect, said)
    for fn in ENTRIES:  # and the well-formed matrix is accepted afterwards
        st, msg = _call(lib, fn, None)
        assert st == 0, (defect, fn[0], st, msg)
