"""TEST INFRASTRUCTURE -- a step-composed twin of the bounds driver's one-call
cut pursuit (pfdr_cp_quadratic_d1_bounds).

The loop of the reference's CP_PFDR_graph_quadratic_d1_bounds
(src/CP_PFDR_graph_quadratic_d1_bounds.cpp:206-973), restated in plain Python
from the reference source in the manner of tests/cp_twin.py, over two backends:

* ``GpuBackend``    -- the library's per-step Python API with host arrays
  (``CPGraph.capacities_bounds``, ``pfdr.cp_reduce`` with its defaults, PFDR
  from zero through ``Lib.quadratic_d1_bounds(..., Ltype=DIAG, L=...)``);
* ``OracleBackend`` -- the C restatement (``Oracle.cp_capacities_bounds``,
  ``Oracle.quadratic_d1_bounds``) around a maxflow the caller passes in;
  N = 0 only (for N = 0 the metric L is rAA itself, :752-753).

What differs from the l1 loop, and is restated here (reference line numbers):

* initialize() (:66-170): the one-component least-squares value rY / rAA
  projected onto [min, max] (:136-139); the residual of the direct case at
  the projected value;
* one cut when min == -inf and max == inf (:392), otherwise two, +1_U then
  -1_U, the second cut's capacities taken before the first cut's activations
  (:427-529);
* PFDR_graph_quadratic_d1_bounds from zero with Ltype = DIAG (:824-836).

The graph has no l1 term; eps (:246), CP_difTol^2 (:305), the iteration that
activates nothing (:535-542), preAt in integers (:648), the merge (:840-863),
the residual (:866-878) and the iterate evolution (:883-901) are cp_twin's,
whose arithmetic the two sources share line for line.
"""
import numpy as np

import cp_twin as T
from cp_twin import canonical, real_eps, seq_sum  # noqa: F401  (re-exported)


class OracleBackend(T.OracleBackend):
    """the C restatement's steps around ``maxflow(tr_cap, r_cap) -> segments``"""

    def __init__(self, o, maxflow, V, Eu, Ev, La_d1, lo, hi):
        super().__init__(o, maxflow, V, Eu, Ev, La_d1, None)
        real = np.asarray(La_d1).dtype.type  # the bounds as the driver holds them
        self.lo, self.hi = float(real(lo)), float(real(hi))

    def capacities(self, cut, positivity=0):
        return self.o.cp_capacities_bounds(cut, self.La_d1, self.lo, self.hi, self.act, self.Cv,
                                           self.rX, self.DfS)

    def pfdr(self, n, Y, A, rEu, rEv, rLa, rL1, positivity, L, rho, condMin, difRcd, difTol,
             itMax):
        X, it, _, _ = self.o.quadratic_d1_bounds(
            np.zeros(L.size, L.dtype), Y, A, n, rEu, rEv, rLa, self.lo, self.hi, 1, L, rho,
            condMin, difRcd, difTol, itMax)
        return X, it


class GpuBackend(T.GpuBackend):
    """the library's per-step Python API, host arrays in and out"""

    def __init__(self, V, Eu, Ev, La_d1, lo, hi):
        super().__init__(V, Eu, Ev, La_d1, None)
        real = np.asarray(La_d1).dtype.type  # the bounds as the driver holds them
        self.lo, self.hi = float(real(lo)), float(real(hi))

    def capacities(self, cut, positivity=0):
        return self.g.capacities_bounds(cut, self.lo, self.hi)

    def pfdr(self, n, Y, A, rEu, rEv, rLa, rL1, positivity, L, rho, condMin, difRcd, difTol,
             itMax):
        X, it, _, _ = self.lib.quadratic_d1_bounds(
            np.zeros(L.size, L.dtype), Y, A, n, rEu, rEv, rLa, self.lo, self.hi,
            Ltype=self.mod.DIAG, L=L, rho=rho, condMin=condMin, difRcd=difRcd, difTol=difTol,
            itMax=itMax)
        return X, it


class Twin(T.Twin):
    """the bounds loop over one backend; ``track``: CP_difTol > 0 or Dif != NULL (:308)"""

    def __init__(self, backend, V, N, Y, A, lo=-np.inf, hi=np.inf, CP_difTol=1e-3, rho=1.0,
                 condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=10000, track=True):
        super().__init__(backend, V, N, Y, A, positivity=0, CP_difTol=CP_difTol, rho=rho,
                         condMin=condMin, difRcd=difRcd, difTol=difTol, itMax=itMax, La_l1=None,
                         track=track)
        real = self.dt.type
        self.lo, self.hi = real(lo), real(hi)
        # T.Twin.iterate takes one cut when `La_l1 is None and not positivity`, else
        # capacities(1) / capacities(2): here two cuts as soon as a bound exists
        # (:392); the backends above ignore the value
        self.positivity = int(not (self.lo == -np.inf and self.hi == np.inf))

    def initialize(self):
        """:66-170 -> rX0 (one value); sets R for N > 0"""
        real, N, V, Y, A = self.dt.type, self.N, self.V, self.Y, self.A
        if N > 0:
            rA = np.zeros(N, self.dt)
            for v in range(V):                                       # :101-109
                rA = rA + A[:, v]
            rY = seq_sum(rA * Y)                                     # :112-116
            rAA = seq_sum(rA * rA)
        else:
            rY = seq_sum(Y)                                          # :120
            if N < 0:
                rAA = seq_sum(np.ascontiguousarray(A.T))             # :124-127, memory order
            elif A is not None:
                rAA = seq_sum(A)                                     # :131
            else:
                rAA = real(V)                                        # :133
        x0 = real(rY / rAA)                                          # :136
        if x0 < self.lo:                                             # :138-139
            x0 = self.lo
        elif x0 > self.hi:
            x0 = self.hi
        if N > 0:
            self.R = Y - rA * x0                                     # :153
        self.rX = np.array([x0], self.dt)
        self.b.set_values(self.rX)
        self._last = (self.Cv.copy(), self.rX.copy())
        return self.rX


def gpu_twin(p, track=True, **over):
    """the twin over the library's steps for a cp_problems.problem("bounds", ...) dict"""
    q = dict(p)
    q.update(over)
    b = GpuBackend(q["V"], q["Eu"], q["Ev"], q["La_d1"], q["lo"], q["hi"])
    return Twin(b, q["V"], q["N"], q["Y"], q["A"], lo=q["lo"], hi=q["hi"],
                CP_difTol=q["CP_difTol"], rho=q["rho"], condMin=q["condMin"], difRcd=q["difRcd"],
                difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"], track=track)
