"""Shared by tests/test_cp_sparse_*.py: the sparse observation operators, the
partitions and a numpy model of the ordered component column sums that the
sparse cut-pursuit entries are checked with.  The reference of every GPU check
is the library's own dense entry on the densified matrix, byte for byte."""
import functools

import numpy as np

from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import blur3x3_csc, uniform

F32, F64 = np.float32, np.float64
MATRICES = ("r300", "blur", "one_row", "holes", "longrun")
PARTITIONS = ("one_id", "one_perm", "bands", "singletons", "mixed")
MIXED_SIZES = (1, 2, 63, 64, 65, 257)  # then the rest: V >= 453
HOLES_EMPTY_ROWS = (5, 77, 199)
HOLES_NEG_ZERO = (77, 33)  # the stored -0.0: alone in its row but for column 20's stored zero


def _random_fill(seed, N, V, fill):
    """(A, stored): ~fill of the entries nonzero in [-1, 1), every column non-empty"""
    idx = np.arange(N * V, dtype=np.uint64).reshape(N, V)
    mask = uniform(seed, idx) < fill
    for v in np.nonzero(~mask.any(axis=0))[0]:
        mask[(7 * v + 3) % N, v] = True
    val = 2.0 * uniform(seed + 1, idx) - 1.0
    val[val == 0] = 0.5
    return np.where(mask, val, 0.0), mask


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> (A float64 N-by-V, stored bool N-by-V); A is zero where nothing is stored"""
    if name == "r300":
        return _random_fill(11, 200, 300, 0.05)
    if name == "blur":
        c = pfdr.CSC(*blur3x3_csc(24, 20), N=480)
        A = c.to_dense()
        return A, A != 0
    if name == "one_row":
        A = (2.0 * uniform(17, np.arange(12, dtype=np.uint64)) - 1.0).reshape(1, 12)
        return A, np.ones((1, 12), bool)
    if name == "holes":
        A, st = (a.copy() for a in matrix("r300"))
        N = A.shape[0]
        for r in HOLES_EMPTY_ROWS:
            A[r], st[r] = 0.0, False
        A[:, 10], st[:, 10] = 0.0, False
        A[50, 10], st[50, 10] = 0.75, True  # a single entry
        st[:, 20] = True                    # fully stored: zeros at the empty rows
        r, v = HOLES_NEG_ZERO
        A[r, v], st[r, v] = -0.0, True
        for v in np.nonzero(~(A != 0).any(axis=0))[0]:  # no column of zeros (0 / 0 downstream)
            A[(7 * v + 4) % 5 + 100, v], st[(7 * v + 4) % 5 + 100, v] = 0.5, True
        return A, st
    if name == "longrun":
        A, st = (a.copy() for a in _random_fill(23, 40, 1200, 0.03))
        A[3, :1000] = 0.1 * (2.0 * uniform(24, np.arange(1000, dtype=np.uint64)) - 1.0) + 0.2
        st[3, :1000] = True
        return A, st
    raise ValueError(name)


def csc(name, dt):
    """the matrix in the dtype, stored zeros (and the -0.0) kept"""
    A, st = matrix(name)
    return pfdr.CSC.from_dense(A.astype(dt), st)


def thinned(A, seed):
    """(A with about half the entries of each column zeroed and at least one
    kept, the mask of the kept ones); A N-by-V"""
    N, V = A.shape
    keep = uniform(seed, np.arange(N * V, dtype=np.uint64).reshape(N, V)) < 0.5
    keep[(5 * np.arange(V) + 1) % N, np.arange(V)] = True
    return np.where(keep, A, 0), keep


def partition(name, V):
    """-> (rVc int32[rV + 1], Vc int32[V]), or None where V is too small"""
    i = np.arange(V)
    if name == "one_id":
        return np.array([0, V], np.int32), i.astype(np.int32)
    if name == "one_perm":  # 7 is coprime to 12, 300, 480 and 1200
        return np.array([0, V], np.int32), ((7 * i + 3) % V).astype(np.int32)
    if name == "bands":     # three components, each in descending vertex order
        cut = [0, V // 3, 2 * (V // 3), V]
        Vc = np.concatenate([i[a:b][::-1] for a, b in zip(cut, cut[1:])])
        return np.array(cut, np.int32), Vc.astype(np.int32)
    if name == "singletons":
        return np.arange(V + 1, dtype=np.int32), i[::-1].astype(np.int32)
    if name == "mixed":
        if V < sum(MIXED_SIZES) + 1:
            return None
        rVc = np.concatenate([[0], np.cumsum(MIXED_SIZES), [V]]).astype(np.int32)
        return rVc, ((11 * i + 5) % V).astype(np.int32)  # 11 is coprime to 480 and 1200
    raise ValueError(name)


def cv_of(rVc, Vc):
    """the component of every vertex"""
    Cv = np.empty(Vc.size, np.int32)
    Cv[Vc] = np.repeat(np.arange(rVc.size - 1), np.diff(rVc))
    return Cv


def model_colsum(c, rVc, Vc, order="list"):
    """rA (rV, N) of a host CSC: every component's stored entries added from +0
    in the CSC's dtype, over the component's vertices in list order (``order`` =
    "list", what the library owes) or in ascending column order ("column")"""
    rV = rVc.size - 1
    rA = np.zeros((rV, c.N), c.dtype)
    for rv in range(rV):
        cols = Vc[rVc[rv]:rVc[rv + 1]]
        if order == "column":
            cols = np.sort(cols)
        a = rA[rv]
        for v in cols:  # a column holds a row once: the adds of one column are independent
            e = slice(c.colptr[v], c.colptr[v + 1])
            a[c.rowidx[e]] = a[c.rowidx[e]] + c.val[e]
    return rA


def model_colsum_dense(A, rVc, Vc):
    """the dense loop: every entry of the columns, zeros included, in list order"""
    rV = rVc.size - 1
    rA = np.zeros((rV, A.shape[0]), A.dtype)
    for rv in range(rV):
        for v in Vc[rVc[rv]:rVc[rv + 1]]:
            rA[rv] = rA[rv] + A[:, v]
    return rA


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def grid_problem(name, dt, nx, ny):
    """a cut-pursuit problem (a cp_problems-style dict of kind "l1") on the
    nx-by-ny grid for the matrix ``name`` (V = nx ny columns): Y = A bands +
    noise, La_d1 = 0.05; A is the dense N-by-V matrix, ``csc`` its CSC"""
    from cp_pfdr_graph_d1_amd.graphs import grid_graph
    A, _ = matrix(name)
    N, V = A.shape
    assert V == nx * ny
    Eu, Ev = grid_graph((nx, ny), 4)
    x0 = np.array([1.0, -0.5, 0.25])[(np.arange(V) % nx) * 3 // nx]
    Y = A @ x0 + 0.05 * (2 * uniform(71, np.arange(N, dtype=np.uint64)) - 1)
    return dict(kind="l1", V=V, E=Eu.size, N=N, K=0, dtype=dt, CP_itMax=8, PFDR_itMax=2000,
                positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3,
                difRcd=0.0, lo=-np.inf, hi=np.inf, al=0.0, Y=Y.astype(dt), A=A.astype(dt),
                csc=csc(name, dt), Eu=Eu, Ev=Ev, La_d1=np.full(Eu.size, 0.05, dt),
                La_l1=np.full(V, 0.02, dt))
