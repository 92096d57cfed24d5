"""TEST INFRASTRUCTURE -- a step-composed twin of the simplex driver's one-call
cut pursuit (pfdr_cp_loss_d1_simplex).

The loop of the reference's CP_PFDR_graph_loss_d1_simplex
(src/CP_PFDR_graph_loss_d1_simplex.cpp), restated in plain
Python from the reference source over a small backend interface, as
tests/cp_twin.py does for the l1 driver:

* ``GpuBackend``    -- the library's per-step Python API with host arrays
  (``pfdr.CPGraph.simplex_*``, ``CPGraph.mincut(arcs=ARCS_FORWARD)``, PFDR
  through ``Lib.loss_d1_simplex`` from the components' own optima);
* ``OracleBackend`` -- the C restatement (``oracle.Oracle("port").cp_simplex_*``
  and its ``loss_d1_simplex``) around a maxflow the caller passes in.

What the twin itself restates (reference line numbers):

* initialize() (:96-116): one component, rP from the reduced observations of
  the one-component state;
* eps (:214-231, as compiled: tests/golden/cp_cases.simplex_eps);
* tracking (:282-306): on when CP_difTol > 0 or Dif is asked for, dif starts
  at max(CP_difTol, 1), the loop ends on CP_it == CP_itMax or dif < CP_difTol;
* one iteration: gradient, K - 1 alpha-expansions, activation (:327-618);
* the iteration that activates nothing (:631-639);
* components, reduced graph, observations, PFDR warm-started at the
  observations' rP with La_f = rLa_f (NULL for al == 0) and no records
  (:643-780), the merge (:782-803);
* the iterate evolution (:808-866) added one by one in ``real``: the mean l1
  change over (v, k) for CP_difTol < 1, the count of vertices whose
  component's first-largest label changed for CP_difTol >= 1;
* the objective (:870-917) added one by one in ``real`` (``objective``), with
  numpy's log where the device has its own: the tests compare Obj against
  f64, not against this.

``Twin.run`` returns (rP0, one record per iteration): Cv, rP, rV, rE, the
reduced problem, the warm start, the number of activated edges, the PFDR
iteration count, dif and the activity after the merge.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from cp_cases import simplex_eps  # noqa: E402


def seq_sum(x):
    """((0 + x[0]) + x[1]) + ... in x's own type"""
    x = np.ascontiguousarray(x).ravel()
    if x.size == 0:
        return x.dtype.type(0)
    return np.add.accumulate(x, dtype=x.dtype)[-1]


def first_max(rP, K):
    """first largest label of every component (:289-298)"""
    return np.argmax(np.asarray(rP).reshape(-1, K), axis=1).astype(np.int32)


def objective(K, al, Q, Cv, rP, rQ, rEu, rEv, rLa):
    """:870-917 in Q's type, every sum sequential in the reference's order"""
    dt = Q.dtype
    real = dt.type
    al = real(al)
    P = np.asarray(rP, dt).reshape(-1, K)
    if al == 0:
        a = seq_sum(-(P.ravel() * np.asarray(rQ, dt).ravel()))
    elif al == 1:
        c = P[Cv] - Q.reshape(-1, K)
        a = seq_sum(c * c) * real(0.5)
    else:
        alK, al1 = al / real(K), real(1) - al
        c = alK + al1 * Q.reshape(-1, K)
        a = seq_sum(c * np.log(c / (alK + al1 * P[Cv])))
    b = real(0)
    if rEu is not None and len(rEu):
        d = np.abs(P[rEu] - P[rEv])
        inner = np.zeros(len(rEu), dt)
        for k in range(K):
            inner = inner + d[:, k]
        b = seq_sum(np.asarray(rLa, dt) * inner)
    return real(a + b)


class OracleBackend:
    """the C restatement's steps around ``maxflow(tr_cap, r_cap) -> segments``"""

    def __init__(self, o, maxflow, K, al, Q, Eu, Ev, La_d1):
        self.o, self.maxflow = o, maxflow
        self.K, self.al = int(K), float(al)
        self.Q = np.ascontiguousarray(Q)
        self.V = self.Q.size // self.K
        self.Eu = np.ascontiguousarray(Eu, np.int32)
        self.Ev = np.ascontiguousarray(Ev, np.int32)
        self.La_d1 = np.ascontiguousarray(La_d1, self.Q.dtype)
        self.act = np.zeros(self.Eu.size, np.uint8)
        self.Cv = np.zeros(self.V, np.int32)
        self.Vc = np.arange(self.V, dtype=np.int32)
        self.rVc = np.array([0, self.V], np.int32)
        self.rP = None

    def set_state(self, active, Cv, Vc, rVc):
        self.act = np.array(active, np.uint8)
        self.Cv, self.Vc, self.rVc = (np.array(x, np.int32) for x in (Cv, Vc, rVc))

    def set_values(self, rP):
        self.rP = np.array(rP, self.Q.dtype)

    def active(self):
        return self.act.copy()

    def observations(self):
        return self.o.cp_simplex_reduced(self.K, self.al, self.Q, self.Vc, self.rVc)

    def gradient(self, eps):
        self.act0 = self.act.copy()
        self.DfS, self.rDi = self.o.cp_simplex_gradient(
            self.K, self.al, self.Q, self.Eu, self.Ev, self.La_d1, self.act0, self.Cv, self.rP,
            eps)
        self.Djv = np.zeros(self.V, np.int32)

    def capacities(self, n):
        return self.o.cp_simplex_capacities(self.K, n, self.Eu, self.Ev, self.La_d1, self.act0,
                                            self.Vc, self.rVc, self.rDi, self.Djv, self.DfS)

    def mincut(self, tr, rc):
        return self.maxflow(tr, rc)

    def expand(self, n, seg):
        self.Djv = self.o.cp_simplex_expand(n, seg, self.Djv)

    def activate(self):
        self.act, n = self.o.cp_simplex_activate(self.Eu, self.Ev, self.Djv, self.act0)
        return n

    def components(self):
        self.Cv, self.Vc, self.rVc = self.o.cp_components(self.V, self.Eu, self.Ev, self.act)
        return self.Cv, self.Vc, self.rVc

    def reduced_graph(self, eps):
        return self.o.cp_reduced_graph(self.V, self.Eu, self.Ev, self.La_d1, None, self.act,
                                       self.Cv, self.Vc, self.rVc, eps)[:3]

    def pfdr(self, rP0, rQ, rEu, rEv, rLa, rLa_f, rho, condMin, difRcd, difTol, itMax):
        P, it, _, _ = self.o.loss_d1_simplex(rP0, rQ, self.K, rEu, rEv, rLa, self.al, rLa_f, rho,
                                             condMin, difRcd, difTol, itMax)
        return P, it

    def merge(self, eps):
        self.act, n = self.o.cp_simplex_merge(self.K, self.Eu, self.Ev, self.Cv, self.rP, eps,
                                              self.act)
        return n

    def close(self):
        pass


class GpuBackend:
    """the library's per-step Python API, host arrays in and out"""

    def __init__(self, K, al, Q, Eu, Ev, La_d1):
        from cp_pfdr_graph_d1_amd import pfdr
        self.mod = pfdr
        self.lib = pfdr.Lib()
        self.K, self.al = int(K), float(al)
        Q = np.ascontiguousarray(Q)
        self.g = pfdr.CPGraph(Q.size // self.K, Eu, Ev, np.ascontiguousarray(La_d1, Q.dtype))
        self.g.simplex_setup(self.K, self.al, Q)

    def set_state(self, active, Cv, Vc, rVc):
        self.g.set_active(active)
        self.g.set_components(Cv, Vc, rVc)

    def set_values(self, rP):
        self.g.simplex_set_values(rP)

    def active(self):
        return self.g.active()

    def observations(self):
        return self.g.simplex_observations()

    def gradient(self, eps):
        self.g.simplex_gradient(eps)

    def capacities(self, n):
        return self.g.simplex_capacities(n)

    def mincut(self, tr, rc):
        return self.g.mincut(tr, rc, arcs=self.mod.ARCS_FORWARD)[0]

    def expand(self, n, seg):
        self.g.simplex_expand(n, seg)

    def activate(self):
        return self.g.simplex_activate()

    def components(self):
        return self.g.components()

    def reduced_graph(self, eps):
        return self.g.reduced_graph(eps)[:3]

    def pfdr(self, rP0, rQ, rEu, rEv, rLa, rLa_f, rho, condMin, difRcd, difTol, itMax):
        P, it, _, _ = self.lib.loss_d1_simplex(rP0, rQ, self.K, rEu, rEv, rLa, self.al, rLa_f,
                                               rho, condMin, difRcd, difTol, itMax)
        return P, it

    def merge(self, eps):
        return self.g.simplex_merge(eps)

    def close(self):
        self.g.close()


class Twin:
    """the loop over one backend; ``track``: CP_difTol > 0 or Dif != NULL (:283)"""

    def __init__(self, backend, K, al, Q, CP_difTol=1e-3, rho=1.0, condMin=0.1, difRcd=0.0,
                 difTol=1e-4, itMax=1000, track=True, obj=False):
        self.b = backend
        self.K, self.al = int(K), float(al)
        self.Q = np.ascontiguousarray(Q)
        self.dt = self.Q.dtype
        self.V = self.Q.size // self.K
        real = self.dt.type
        self.CP_difTol = real(CP_difTol)
        self.eps = simplex_eps(real, self.V, CP_difTol, difTol)          # :214-231
        self.par = dict(rho=rho, condMin=condMin, difRcd=difRcd, difTol=difTol, itMax=itMax)
        self.track = bool(track) or CP_difTol > 0
        self.labels = CP_difTol >= 1
        self.want_obj = bool(obj)
        self.rV, self.rE = 1, 0
        self.Cv = np.zeros(self.V, np.int32)
        self.rP = None

    def _remember(self):
        vals = first_max(self.rP, self.K) if self.labels else self.rP.copy()
        self._last = (self.Cv.copy(), vals)

    def initialize(self):
        """:96-116 -> rP0 (K values) and, when asked, the functional there"""
        rP, rQ, _ = self.b.observations()
        self.rP = np.ascontiguousarray(rP, self.dt)
        self.b.set_values(self.rP)
        self._remember()
        self.obj0 = (objective(self.K, self.al, self.Q, self.Cv, self.rP, rQ, None, None, None)
                     if self.want_obj else None)
        return self.rP

    def restart(self, state):
        """warm restart from a recorded state (active, Cv, Vc, rVc, rP)"""
        self.b.set_state(state["active"], state["Cv"], state["Vc"], state["rVc"])
        self.rP = np.array(state["rP"], self.dt)
        self.b.set_values(self.rP)
        self.Cv = np.array(state["Cv"], np.int32)
        self.rV = self.rP.size // self.K
        self._remember()

    def iterate(self):
        b, K, real = self.b, self.K, self.dt.type
        eps = float(self.eps)
        rec = {}
        b.gradient(eps)                                                  # :327-376, :522-536
        segs = []
        for n in range(1, K):                                            # :539-606
            tr, rc = b.capacities(n)
            seg = b.mincut(tr, rc)
            b.expand(n, seg)
            segs.append(seg)
        w = b.activate()                                                 # :608-618
        rec.update(segments=segs, activated=w)
        if w == 0:                                                       # :631-639
            rec.update(Cv=self.Cv.copy(), rP=self.rP.copy(), rV=self.rV, rE=self.rE,
                       reduced=None, pfdr_it=None, active=b.active(),
                       dif=real(0) if self.track else None, obj=None)
            return rec
        Cv, Vc, rVc = b.components()                                     # :645-676
        rV = rVc.size - 1
        rEu, rEv, rLa = b.reduced_graph(eps)                             # :678-731
        rP0, rQ, rLa_f = b.observations()                                # :733-766
        rP, pit = b.pfdr(rP0, rQ, rEu, rEv, rLa, rLa_f, **self.par)      # :778-780
        rP = np.ascontiguousarray(rP, self.dt)
        b.set_values(rP)
        b.merge(eps)                                                     # :782-803
        dif = None
        if self.track:                                                   # :808-866
            Cv_, vals_ = self._last
            if self.labels:
                lab = first_max(rP, K)
                dif = seq_sum((lab[Cv] != vals_[Cv_]).astype(self.dt))
            else:
                d = np.abs(rP.reshape(-1, K)[Cv] - vals_.reshape(-1, K)[Cv_])
                dif = seq_sum(d) / real(self.V)
        self.Cv, self.rP, self.rV, self.rE = Cv.copy(), rP, rV, rEu.size
        if self.track:
            self._remember()
        obj = (objective(K, self.al, self.Q, Cv, rP, rQ, rEu, rEv, rLa)
               if self.want_obj else None)
        rec.update(Cv=self.Cv.copy(), rP=rP.copy(), rV=rV, rE=rEu.size, Vc=Vc.copy(),
                   rVc=rVc.copy(), reduced=dict(rEu=rEu, rEv=rEv, rLa_d1=rLa, rQ=rQ, rLa_f=rLa_f,
                                                rP0=rP0),
                   pfdr_it=pit, active=b.active(), dif=dif, obj=obj)
        return rec

    def run(self, CP_itMax):
        """from the initial state -> (rP0, [one record per iteration]); the
        loop ends like the reference's (:322): CP_it == CP_itMax or dif < CP_difTol"""
        real = self.dt.type
        rP0 = self.initialize().copy()
        dif = self.CP_difTol if self.CP_difTol > real(1) else real(1)    # :282
        recs = []
        while not (len(recs) == CP_itMax or dif < self.CP_difTol):       # :322
            rec = self.iterate()
            if self.track:
                dif = rec["dif"]
            recs.append(rec)
        return rP0, recs


def gpu_twin(p, track=True, obj=False, **over):
    """the twin over the library's steps for a cp_problems.problem("simplex") dict"""
    q = dict(p)
    q.update(over)
    b = GpuBackend(q["K"], q["al"], q["Y"], q["Eu"], q["Ev"], q["La_d1"])
    return Twin(b, q["K"], q["al"], q["Y"], CP_difTol=q["CP_difTol"], rho=q["rho"],
                condMin=q["condMin"], difRcd=q["difRcd"], difTol=q["PFDR_difTol"],
                itMax=q["PFDR_itMax"], track=track, obj=obj)
