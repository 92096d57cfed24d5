"""TEST INFRASTRUCTURE for tests/test_cp_reduced_sparse_*.py: cut pursuit with
the reduced operator kept sparse (pfdr_cp_solver_set_reduced,
pfdr_cp_reduce_csc_sparse_*).

* the problems and solvers of tests/test_cp_sparse_gpu.py with the ``reduced``
  keyword, and a problem whose matrix has a zero column on an isolated vertex;
* ``SparseBackend``: cp_twin.GpuBackend taking the steps the sparse mode takes
  -- the gradient over the CSC, ``cp_reduce(..., reduced="sparse")`` on a direct
  iteration whose columns all have a positive norm (the dense direct branch
  otherwise), and PFDR on that CSC -- so that ``cp_twin.Twin``, unchanged,
  composes the sparse-mode run from the public steps;
* the two measured figures that the tolerance tests assert ten times.
"""
import functools

import numpy as np

import cp_run_cases
import cp_sparse_cases as SC
import cp_twin as T
from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import grid_graph, uniform

F32, F64 = np.float32, np.float64
THIN_SEED = 81
FLAVOURS = {"l1": dict(), "l1_pos": dict(positivity=1), "duplex": dict(duplex=True),
            "bounds": dict(bounds=True)}
BOX = dict(lo=-0.3, hi=0.8)
PROBLEMS = ("direct12", "direct12_thin", "blur")

# Measured on an MI355X over the cases of the tests named ("Sparse
# reduced operator"); the tests print the figure again and assert ten times it.
#   L of the sparse step against L of the dense cp_reduce, largest relative
#   difference over test_reduce's cases (two power-method estimates of c):
#   5.391e-3 in f32 and in f64, at ("holes", "identity"); ten times it is above
#   the cap, so the cap of 1e-2 is what the test asserts
L_REL_MEASURED = 5.391e-3
#   the functional (f64 numpy) at the sparse mode's final state against the
#   dense mode's, largest relative gap over test_solver's problems and flavours:
#   2.469e-8 in f32 (3.201e-9 in f64), both at ("direct12_thin", "bounds")
OBJ_GAP_MEASURED = 2.469e-8


def bound(measured, cap=None):
    """ten times the measured figure (``cap`` at most)"""
    b = 10.0 * measured
    return b if cap is None else min(b, cap)


@functools.lru_cache(maxsize=None)
def problem(name, dt):
    """-> cp_problems-style dict with the dense N-by-V ``A`` and its ``csc``
    (tests/test_cp_sparse_gpu.py's problems), or "zero_column" """
    if name == "zero_column":
        return zero_column_problem(dt)
    if name in SC.MATRICES:
        nx, ny = {"r300": (20, 15), "blur": (24, 20)}[name]
        return SC.grid_problem(name, dt, nx, ny)
    base, _, thin = name.partition("_")
    p = dict(cp_run_cases.problem(base, dt))
    A = np.ascontiguousarray(p["A"].reshape(p["V"], p["N"]).T)  # N-by-V
    if thin:
        A, _ = SC.thinned(A, THIN_SEED)
        p["csc"] = pfdr.CSC.from_dense(A)
    else:
        p["csc"] = pfdr.CSC.from_dense(A, np.ones(A.shape, bool))
    p["A"] = A
    return p


ZERO_V, ZERO_AT = 30, 17


def zero_column_matrix(dt):
    """2-by-30, every entry stored but column 17, which stores none"""
    N, V = 2, ZERO_V
    A = 2.0 * uniform(41, np.arange(N * V, dtype=np.uint64).reshape(N, V)) - 1.0
    A[np.abs(A) < 0.05] = 0.5
    A[:, ZERO_AT] = 0.0
    st = np.ones((N, V), bool)
    st[:, ZERO_AT] = False
    return A.astype(dt), st


def zero_column_problem(dt):
    """the 6-by-5 grid with vertex 17 cut off from it and column 17 of A zero:
    vertex 17 is a component of its own from the first cut on, and with N = 2
    every iteration is a direct one (2 N pit / (N + pit) = 3 for pit = 200, and
    a cut leaves vertex 17 and at least two more components)"""
    A, st = zero_column_matrix(dt)
    N, V = A.shape
    Eu, Ev = grid_graph((6, 5), 4)
    keep = (Eu != ZERO_AT) & (Ev != ZERO_AT)
    Eu, Ev = Eu[keep], Ev[keep]
    x0 = np.array([1.0, -0.5, 0.25])[(np.arange(V) % 6) // 2]
    Y = A.astype(F64) @ x0 + 0.05 * (2 * uniform(42, np.arange(N, dtype=np.uint64)) - 1)
    return dict(kind="l1", V=V, E=Eu.size, N=N, K=0, dtype=dt, CP_itMax=4, PFDR_itMax=200,
                positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3,
                difRcd=0.0, lo=-np.inf, hi=np.inf, al=0.0, Y=Y.astype(dt), A=A,
                csc=pfdr.CSC.from_dense(A, st), Eu=Eu, Ev=Ev,
                La_d1=np.full(Eu.size, 0.01, dt), La_l1=np.full(V, 0.002, dt))


def solver(p, flavour, reduced="dense", device=False, dense_A=False):
    """a CPSolver of the flavour on the problem's CSC (or, dense_A, its matrix)"""
    f = FLAVOURS[flavour]
    kw = dict(BOX) if f.get("bounds") else dict(
        La_l1=p["La_l1"], positivity=f.get("positivity", 0), duplex=f.get("duplex", False))
    A = np.asfortranarray(p["A"]).ravel(order="F") if dense_A else p["csc"]
    arrs = [p["Y"], p["Eu"], p["Ev"], p["La_d1"]]
    if device:
        import torch
        arrs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
        A = A.to_device()
        if "La_l1" in kw:
            kw["La_l1"] = torch.from_numpy(kw["La_l1"]).cuda()
    return pfdr.CPSolver("bounds" if f.get("bounds") else "l1", *arrs, A=A, N=p["N"],
                         reduced=reduced, **kw)


def params(p, **over):
    q = dict(CP_difTol=p["CP_difTol"], CP_itMax=p["CP_itMax"], rho=p["rho"],
             condMin=p["condMin"], difRcd=p["difRcd"], difTol=p["PFDR_difTol"],
             itMax=p["PFDR_itMax"])
    q.update(over)
    return q


ZERO_NORM = "has norm 0"  # the library's words for a reduced column it refuses


class SparseBackend(T.GpuBackend):
    """the steps of a sparse-mode iteration; counts what reduced_stats() counts"""

    def __init__(self, csc, *a, **kw):
        super().__init__(*a, **kw)
        self.csc = csc
        self.kept = None  # the sparse rA of the iteration under way
        self.sparse_its = self.dense_direct_its = self.max_rnnz = 0

    def gradient(self, N, A, Y, R):
        self.g.gradient(N, self.csc, None, R)

    def reduce(self, N, A, Y, preAt):
        self.kept = None
        if preAt:
            return self.mod.cp_reduce(N, self.csc, Y, self.rVc, self.Vc, preAt=True)
        try:
            red = self.mod.cp_reduce(N, self.csc, Y, self.rVc, self.Vc, preAt=False,
                                     reduced="sparse")
        except self.mod.PFDRError as e:  # a column with l = 0: the dense direct branch
            if ZERO_NORM not in str(e):
                raise
            self.dense_direct_its += 1
            return self.mod.cp_reduce(N, self.csc, Y, self.rVc, self.Vc, preAt=False)
        self.kept = red["rA"]
        self.sparse_its += 1
        self.max_rnnz = max(self.max_rnnz, self.kept.nnz)
        return dict(red, rA=self.kept.to_dense())  # for the twin's residual loop

    def pfdr(self, n, Y, A, *rest, **kw):
        if n > 0 and self.kept is not None:
            A = self.kept
        return super().pfdr(n, Y, A, *rest, **kw)


def twin(p, flavour):
    """cp_twin.Twin over a SparseBackend for the problem and the flavour"""
    f = FLAVOURS[flavour]
    bounds = bool(f.get("bounds"))
    kind = "bounds" if bounds else "duplex" if f.get("duplex") else "l1"
    La_l1 = None if bounds else p["La_l1"]
    box = BOX if bounds else dict(lo=-np.inf, hi=np.inf)
    b = SparseBackend(p["csc"], p["V"], p["Eu"], p["Ev"], p["La_d1"], La_l1, kind, box["lo"],
                      box["hi"])
    return T.Twin(b, p["V"], p["N"], p["Y"], np.asfortranarray(p["A"]).ravel(order="F"),
                  positivity=f.get("positivity", 0), CP_difTol=p["CP_difTol"], rho=p["rho"],
                  condMin=p["condMin"], difRcd=p["difRcd"], difTol=p["PFDR_difTol"],
                  itMax=p["PFDR_itMax"], La_l1=La_l1, track=True)


def functional(p, flavour, Cv, rX):
    """1/2 ||Y - A x||^2 + sum La_d1 |x_u - x_v| (+ sum La_l1 |x_v|) at x = rX[Cv], f64"""
    x = np.asarray(rX, F64)[Cv]
    r = p["Y"].astype(F64) - p["A"].astype(F64) @ x
    F = 0.5 * float(r @ r)
    F += float(np.sum(p["La_d1"].astype(F64) * np.abs(x[p["Eu"]] - x[p["Ev"]])))
    if not FLAVOURS[flavour].get("bounds"):
        F += float(np.sum(p["La_l1"].astype(F64) * np.abs(x)))
    return F


def stored_model(c, rVc, Vc):
    """bool N-by-rV: A stores some entry A[n, v] with v in component rv"""
    st = np.zeros((c.N, c.V), bool)
    st[c.rowidx, np.repeat(np.arange(c.V), np.diff(c.colptr))] = True
    return np.stack([st[:, Vc[rVc[rv]:rVc[rv + 1]]].any(axis=1) for rv in range(rVc.size - 1)],
                    axis=1)
