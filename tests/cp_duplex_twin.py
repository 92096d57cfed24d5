"""TEST INFRASTRUCTURE -- a step-composed twin of the duplex driver's one-call
cut pursuit (pfdr_cp_quadratic_d1_l1_duplex).

The loop of the reference's CP_PFDR_graph_quadratic_d1_l1_duplex
(src/CP_PFDR_graph_quadratic_d1_l1_duplex.cpp), which differs from the l1
driver's source in the graph and the cut only: tests/cp_twin.py's loop with the
cut block replaced by one two-layer cut (:469-545),

    gradient -> capacities_duplex -> two-layer maxflow -> activate_duplex,

over two backends:

* ``GpuBackend``    -- the library's per-step Python API with host arrays
  (``CPGraph.capacities_duplex``, ``mincut_duplex``, ``activate_duplex``);
* ``OracleBackend`` -- the C restatement (``Oracle.cp_capacities_duplex``,
  ``Oracle.cp_activate_duplex``) around a maxflow
  ``maxflow(tr_cap[2V], r_link[V], r_cap[E]) -> segments[2V]`` the caller
  passes in; N = 0 only.

cp_twin.Twin.iterate takes its single-cut block -- capacities(0, 0), mincut,
activate -- when ``La_l1 is None and not positivity``.  The duplex Twin runs
that very block for its one cut: during iterate() it hides the l1 term and
positivity from cp_twin's branch, and the backends here, which hold both
themselves, answer capacities / mincut / activate with the two-layer steps and
hand PFDR the true positivity.  Everything else -- initialize(), eps, the
iteration that activates nothing, preAt, PFDR from zero, merge, residual,
iterate evolution, stopping rule -- is cp_twin's, unchanged.

The differentiable case (no l1 term, no positivity) is the l1 driver's
single-cut path, as in the entry.
"""
import numpy as np

import cp_twin as T
from cp_twin import canonical, real_eps, seq_sum  # noqa: F401  (re-exported)


class _DuplexSteps:
    """the three steps of the cut block, two-layer when ``self.two``"""

    def capacities(self, cut, positivity=0):
        if not self.two:
            return super().capacities(cut, positivity)
        tr, link, rc = self._capacities_duplex()
        return tr, (link, rc)

    def mincut(self, tr, caps):
        if not self.two:
            return super().mincut(tr, caps)
        return self._mincut_duplex(tr, *caps)

    def activate(self, seg):
        if not self.two:
            return super().activate(seg)
        return self._activate_duplex(seg)

    def pfdr(self, n, Y, A, rEu, rEv, rLa, rL1, positivity, *a, **kw):
        return super().pfdr(n, Y, A, rEu, rEv, rLa, rL1, self.positivity, *a, **kw)


class OracleBackend(_DuplexSteps, T.OracleBackend):
    def __init__(self, o, maxflow, V, Eu, Ev, La_d1, La_l1, positivity):
        super().__init__(o, maxflow, V, Eu, Ev, La_d1, La_l1)
        self.positivity = int(positivity)
        self.two = La_l1 is not None or bool(positivity)

    def _capacities_duplex(self):
        return self.o.cp_capacities_duplex(self.La_d1, self.La_l1, self.positivity, self.act,
                                           self.Cv, self.rX, self.DfS)

    def _mincut_duplex(self, tr, link, rc):
        return self.maxflow(tr, link, rc)

    def _activate_duplex(self, seg):
        self.act, n = self.o.cp_activate_duplex(self.V, self.Eu, self.Ev, seg, self.act)
        return n


class GpuBackend(_DuplexSteps, T.GpuBackend):
    def __init__(self, V, Eu, Ev, La_d1, La_l1, positivity):
        super().__init__(V, Eu, Ev, La_d1, La_l1)
        self.positivity = int(positivity)
        self.two = La_l1 is not None or bool(positivity)

    def _capacities_duplex(self):
        return self.g.capacities_duplex(self.positivity)

    def _mincut_duplex(self, tr, link, rc):
        return self.g.mincut_duplex(tr, link, rc)[0]

    def _activate_duplex(self, seg):
        return self.g.activate_duplex(seg)


class Twin(T.Twin):
    """the duplex loop over one of the backends above"""

    def iterate(self):
        if not self.b.two:
            return super().iterate()
        keep = (self.La_l1, self.positivity)
        self.La_l1, self.positivity = None, 0  # cp_twin's single-cut block (see above)
        try:
            rec = super().iterate()
        finally:
            self.La_l1, self.positivity = keep
        assert len(rec["segments"]) == 1 and rec["segments"][0].size == 2 * self.V
        return rec


def gpu_twin(p, track=True, **over):
    """the twin over the library's steps for a cp_problems.problem("duplex", ...) dict"""
    q = dict(p)
    q.update(over)
    b = GpuBackend(q["V"], q["Eu"], q["Ev"], q["La_d1"], q["La_l1"], q["positivity"])
    return Twin(b, q["V"], q["N"], q["Y"], q["A"], positivity=q["positivity"],
                CP_difTol=q["CP_difTol"], rho=q["rho"], condMin=q["condMin"], difRcd=q["difRcd"],
                difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"], La_l1=q["La_l1"], track=track)
