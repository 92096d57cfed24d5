"""TEST INFRASTRUCTURE -- a step-composed twin of the one-call quadratic cut
pursuits, with the ``flavour`` of the driver it mirrors (QuadDriver,
csrc/pfdr_cutpursuit.hip): "l1", "duplex" or "bounds".

The loop of the reference's CP_PFDR_graph_quadratic_d1_l1
(src/CP_PFDR_graph_quadratic_d1_l1.cpp), restated in plain
Python from the reference source over a small backend interface:

* ``GpuBackend``    -- the library's per-step Python API with host arrays
  (``pfdr.CPGraph``, ``pfdr.cp_reduce`` with its defaults, PFDR from zero
  through ``Lib.quadratic_d1_l1(..., Ltype=DIAG, L=...)``);
* ``OracleBackend`` -- the C restatement (``oracle.Oracle("port")``) around a
  maxflow the caller passes in, ``maxflow(tr_cap, r_cap) -> segments`` and, for
  a two-layer cut, ``maxflow(tr_cap[2V], r_link[V], r_cap[E]) -> segments[2V]``;
  N = 0 only (the restatement has no operator norm, and for N = 0 the metric L
  is rAA itself, :775-776).

The flavour is used where QuadDriver uses it, and nowhere else:

* "duplex": CP_PFDR_graph_quadratic_d1_l1_duplex
  (src/CP_PFDR_graph_quadratic_d1_l1_duplex.cpp), which differs from the l1
  driver's source in the graph and the cut only.  With an l1 term or positivity
  the cut block is one two-layer cut (:469-545), gradient -> capacities_duplex
  -> two-layer maxflow -> activate_duplex; the differentiable case is the l1
  driver's single cut, as in the entry.
* "bounds": CP_PFDR_graph_quadratic_d1_bounds
  (src/CP_PFDR_graph_quadratic_d1_bounds.cpp:206-973).  initialize() (:66-170)
  projects the one-component least-squares value rY / rAA onto [min, max]
  (:136-139), and the residual of the direct case is taken at the projected
  value; one cut when min == -inf and max == inf (:392), otherwise two, +1_U
  then -1_U, the second cut's capacities taken before the first cut's
  activations (:427-529), from ``capacities_bounds``; PFDR is
  PFDR_graph_quadratic_d1_bounds from zero with Ltype = DIAG (:824-836,
  ``quadratic_d1_bounds``); for N = 0 L is rAA (:752-753).  The graph has no l1
  term; eps (:246), CP_difTol^2 (:305), the iteration that activates nothing
  (:535-542), preAt in integers (:648), the merge (:840-863), the residual
  (:866-878) and the iterate evolution (:883-901) are the l1 loop's, whose
  arithmetic the two sources share line for line.

What the twin itself restates (l1 reference line numbers):

* initialize() (:94-175): the one-component solution, every sum added one by
  one in ``real`` (the reference built without OpenMP), the residual
  R = Y - rA x0 of the direct case;
* eps (:252) and CP_difTol^2 (:311), in ``real``;
* the cut block as QuadDriver::loop spells it: the two-layer cut, one cut
  (differentiable), or two, the second cut's capacities taken before the first
  cut's activations (:402-560);
* the iteration that activates nothing (:556-563);
* preAt = N <= 0 or rV < (2 N PFDR_it) / (N + PFDR_it) in integers, PFDR_it
  from the previous PFDR call and PFDR_itMax before the first (:308, :671);
* PFDR from zero with Ltype = DIAG (:847-859), the merge (:863-886);
* the residual R = Y - rA rX, rv ascending, in ``real`` (:889-901);
* the iterate evolution (:905-923) in ``real`` in the reference's order --
  only because the stopping rule (:335) reads it; ``Obj`` is not formed.  The
  tests check the entry's Obj / Dif against f64, not against this.

``Twin.run`` returns one record per iteration: Cv, rX, rV, rE, the reduced
graph, whether preAt was taken, the number of activated edges, the PFDR
iteration count, dif and the activity after the merge.
"""
import numpy as np


def seq_sum(x):
    """((0 + x[0]) + x[1]) + ... in x's own type"""
    x = np.ascontiguousarray(x).ravel()
    if x.size == 0:
        return x.dtype.type(0)
    return np.add.accumulate(x, dtype=x.dtype)[-1]


def real_eps(dt, CP_difTol):
    """:235-252: CP_difTol if 0 < CP_difTol < machine eps (both in real), else it"""
    dt = np.dtype(dt).type
    m = dt(np.finfo(dt).eps)
    c = dt(CP_difTol)
    return c if dt(0) < c < m else m


def matrix(N, V, A, dt):
    """the problem's A as the steps take it: (N, V) for N > 0 and (V, V) for
    N < 0 over the caller's column-major memory, the diagonal or None for N = 0"""
    if A is None:
        return None
    A = np.ascontiguousarray(A, dt)
    if N > 0:
        return A.reshape(V, N).T
    if N < 0:
        return A.reshape(V, V).T
    return A


class OracleBackend:
    """the C restatement's steps around ``maxflow``; lo, hi: the box of "bounds" """

    def __init__(self, o, maxflow, V, Eu, Ev, La_d1, La_l1=None, flavour="l1", lo=-np.inf,
                 hi=np.inf):
        self.o, self.maxflow, self.flavour = o, maxflow, flavour
        real = np.asarray(La_d1).dtype.type  # the bounds as the driver holds them
        self.lo, self.hi = real(lo), real(hi)
        self.V = int(V)
        self.Eu = np.ascontiguousarray(Eu, np.int32)
        self.Ev = np.ascontiguousarray(Ev, np.int32)
        self.La_d1, self.La_l1 = La_d1, La_l1
        self.act = np.zeros(self.Eu.size, np.uint8)
        self.Cv = np.zeros(self.V, np.int32)
        self.Vc = np.arange(self.V, dtype=np.int32)
        self.rVc = np.array([0, self.V], np.int32)
        self.rX = self.DfS = None

    def set_state(self, active, Cv, Vc, rVc):
        self.act = np.array(active, np.uint8)
        self.Cv, self.Vc, self.rVc = (np.array(x, np.int32) for x in (Cv, Vc, rVc))

    def set_values(self, rX):
        self.rX = np.array(rX)

    def active(self):
        return self.act.copy()

    def gradient(self, N, A, Y, R):
        self.DfS = self.o.cp_gradient(N, self.V, A, Y, R, self.Eu, self.Ev, self.La_d1,
                                      self.La_l1, self.act, self.Cv, self.Vc, self.rVc, self.rX)

    def capacities(self, cut, positivity):
        if self.flavour == "bounds":
            return self.o.cp_capacities_bounds(cut, self.La_d1, float(self.lo), float(self.hi),
                                               self.act, self.Cv, self.rX, self.DfS)
        return self.o.cp_capacities(cut, self.La_d1, self.La_l1, positivity, self.act, self.Cv,
                                    self.rX, self.DfS)

    def capacities_duplex(self, positivity):
        """-> (tr[2V], link[V], rc[E])"""
        return self.o.cp_capacities_duplex(self.La_d1, self.La_l1, positivity, self.act, self.Cv,
                                           self.rX, self.DfS)

    def mincut(self, tr, rc):
        return self.maxflow(tr, rc)

    def mincut_duplex(self, tr, link, rc):
        return self.maxflow(tr, link, rc)

    def activate(self, seg):
        self.act, n = self.o.cp_activate(self.Eu, self.Ev, seg, self.act)
        return n

    def activate_duplex(self, seg):
        self.act, n = self.o.cp_activate_duplex(self.V, self.Eu, self.Ev, seg, self.act)
        return n

    def components(self):
        self.Cv, self.Vc, self.rVc = self.o.cp_components(self.V, self.Eu, self.Ev, self.act)
        return self.Cv, self.Vc, self.rVc

    def reduced_graph(self, eps):
        return self.o.cp_reduced_graph(self.V, self.Eu, self.Ev, self.La_d1, self.La_l1, self.act,
                                       self.Cv, self.Vc, self.rVc, eps)

    def reduce(self, N, A, Y, preAt):
        if N != 0:
            raise NotImplementedError("oracle backend: N = 0 only (no operator norm)")
        red = self.o.cp_reduce(0, A, Y, self.rVc, self.Vc)
        red["L"] = red["rAA"]  # :775-776
        return red

    def pfdr(self, n, Y, A, rEu, rEv, rLa, rL1, positivity, L, rho, condMin, difRcd, difTol,
             itMax):
        own = (float(self.lo), float(self.hi)) if self.flavour == "bounds" else (rL1, positivity)
        fn = self.o.quadratic_d1_bounds if self.flavour == "bounds" else self.o.quadratic_d1_l1
        X, it, _, _ = fn(np.zeros(L.size, L.dtype), Y, A, n, rEu, rEv, rLa, *own, 1, L, rho,
                         condMin, difRcd, difTol, itMax)
        return X, it

    def merge(self, eps, difTol):
        self.act, n = self.o.cp_merge(self.Eu, self.Ev, self.Cv, self.rX, eps, difTol, self.act)
        return n

    def close(self):
        pass


class GpuBackend:
    """the library's per-step Python API, host arrays in and out"""

    def __init__(self, V, Eu, Ev, La_d1, La_l1=None, flavour="l1", lo=-np.inf, hi=np.inf):
        from cp_pfdr_graph_d1_amd import pfdr
        self.mod, self.flavour = pfdr, flavour
        real = np.asarray(La_d1).dtype.type  # the bounds as the driver holds them
        self.lo, self.hi = real(lo), real(hi)
        self.lib = pfdr.Lib()
        self.g = pfdr.CPGraph(V, Eu, Ev, La_d1, La_l1)

    def set_state(self, active, Cv, Vc, rVc):
        self.g.set_active(active)
        self.g.set_components(Cv, Vc, rVc)

    def set_values(self, rX):
        self.g.set_values(rX)

    def active(self):
        return self.g.active()

    def gradient(self, N, A, Y, R):
        self.g.gradient(N, A, None if N > 0 else Y, R)

    def capacities(self, cut, positivity):
        if self.flavour == "bounds":
            return self.g.capacities_bounds(cut, float(self.lo), float(self.hi))
        return self.g.capacities(cut, positivity)

    def capacities_duplex(self, positivity):
        """-> (tr[2V], link[V], rc[E])"""
        return self.g.capacities_duplex(positivity)

    def mincut(self, tr, rc):
        return self.g.mincut(tr, rc)[0]

    def mincut_duplex(self, tr, link, rc):
        return self.g.mincut_duplex(tr, link, rc)[0]

    def activate(self, seg):
        return self.g.activate(seg)

    def activate_duplex(self, seg):
        return self.g.activate_duplex(seg)

    def components(self):
        self.Cv, self.Vc, self.rVc = self.g.components()
        return self.Cv, self.Vc, self.rVc

    def reduced_graph(self, eps):
        return self.g.reduced_graph(eps)

    def reduce(self, N, A, Y, preAt):
        return self.mod.cp_reduce(N, A, Y, self.rVc, self.Vc, preAt=preAt)

    def pfdr(self, n, Y, A, rEu, rEv, rLa, rL1, positivity, L, rho, condMin, difRcd, difTol,
             itMax):
        own = (float(self.lo), float(self.hi)) if self.flavour == "bounds" else (rL1, positivity)
        fn = self.lib.quadratic_d1_bounds if self.flavour == "bounds" else self.lib.quadratic_d1_l1
        X, it, _, _ = fn(np.zeros(L.size, L.dtype), Y, A, n, rEu, rEv, rLa, *own,
                         Ltype=self.mod.DIAG, L=L, rho=rho, condMin=condMin, difRcd=difRcd,
                         difTol=difTol, itMax=itMax)
        return X, it

    def merge(self, eps, difTol):
        return self.g.merge(eps, difTol)

    def close(self):
        self.g.close()


class Twin:
    """the loop over one backend, whose flavour and box it takes; ``track``:
    CP_difTol > 0 or Dif != NULL (:314)"""

    def __init__(self, backend, V, N, Y, A, positivity=0, CP_difTol=1e-3, rho=1.0,
                 condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=10000, La_l1=None, track=True):
        self.b = backend
        self.V, self.N = int(V), int(N)
        self.Y = np.ascontiguousarray(Y)
        self.dt = self.Y.dtype
        self.A = matrix(self.N, self.V, A, self.dt)
        self.La_l1 = None if La_l1 is None else np.ascontiguousarray(La_l1, self.dt)
        self.positivity = int(positivity)
        real = self.dt.type
        self.flavour, self.lo, self.hi = backend.flavour, real(backend.lo), real(backend.hi)
        self.CP_difTol = real(CP_difTol)
        self.eps = real_eps(self.dt, CP_difTol)                      # :252
        self.difTol2 = self.CP_difTol * self.CP_difTol               # :311
        self.par = dict(rho=rho, condMin=condMin, difRcd=difRcd, difTol=difTol, itMax=itMax)
        self.track = bool(track)        # CP_difTol > 0 or Dif != NULL (:314)
        self.PFDR_it = int(itMax)       # :308
        self.R = None
        self.rV, self.rE = 1, 0
        self.Cv = np.zeros(self.V, np.int32)
        self.rX = None

    # ------------------------------------------------------ initialize() --
    def initialize(self):
        """:94-175 -> rX0 (one value); sets R for N > 0"""
        real, N, V, Y, A = self.dt.type, self.N, self.V, self.Y, self.A
        if N > 0:
            rA = np.zeros(N, self.dt)
            for v in range(V):                                       # :101-109
                rA = rA + A[:, v]
            rY = seq_sum(rA * Y)                                     # :111-115
            rAA = seq_sum(rA * rA)
        else:
            rY = seq_sum(Y)                                          # :118
            if N < 0:
                rAA = seq_sum(np.ascontiguousarray(A.T))             # :121-124, memory order
            elif A is not None:
                rAA = seq_sum(A)                                     # :127
            else:
                rAA = real(V)                                        # :129
        rL1 = seq_sum(self.La_l1) if self.La_l1 is not None else real(0)
        if self.flavour == "bounds":                                 # bounds :136-139
            x0 = real(rY / rAA)
            x0 = self.lo if x0 < self.lo else self.hi if x0 > self.hi else x0
        elif rY > rL1:                                               # :138-140
            x0 = (rY - rL1) / rAA
        elif not self.positivity and rY < -rL1:
            x0 = (rY + rL1) / rAA
        else:
            x0 = real(0)
        if N > 0:
            self.R = Y - rA * x0                                     # :154
        self.rX = np.array([x0], self.dt)
        self.b.set_values(self.rX)
        self._last = (self.Cv.copy(), self.rX.copy())
        return self.rX

    def restart(self, state, R=None):
        """warm restart from a recorded state (active, Cv, Vc, rVc, rX) (:296-303)"""
        self.b.set_state(state["active"], state["Cv"], state["Vc"], state["rVc"])
        self.rX = np.array(state["rX"], self.dt)
        self.b.set_values(self.rX)
        self.Cv = np.array(state["Cv"], np.int32)
        self.rV = self.rX.size
        self.R = R
        self._last = (self.Cv.copy(), self.rX.copy())

    # ------------------------------------------------------ one iteration --
    def iterate(self):
        b, N, real = self.b, self.N, self.dt.type
        rec = {}
        b.gradient(N, self.A, self.Y, self.R if N > 0 else None)     # :339-400
        segs = []
        two = self.flavour == "duplex" and (self.La_l1 is not None or bool(self.positivity))
        if self.flavour == "bounds":                                 # bounds :392
            one = self.lo == -np.inf and self.hi == np.inf
        else:
            one = self.La_l1 is None and not self.positivity
        if two:                                                      # duplex :469-545
            tr, link, rc = b.capacities_duplex(self.positivity)
            segs.append(b.mincut_duplex(tr, link, rc))
            w = b.activate_duplex(segs[0])
        elif one:                                                    # :402-440
            tr, rc = b.capacities(0, 0)
            segs.append(b.mincut(tr, rc))
            w = b.activate(segs[0])
        else:                                                        # :441-550
            tr, rc = b.capacities(1, self.positivity)
            segs.append(b.mincut(tr, rc))
            # the second cut's capacities read the activity before the first
            # cut's activations (the reference activates after both maxflows'
            # capacities are set, :521-548)
            tr, rc = b.capacities(2, self.positivity)
            w = b.activate(segs[0])
            segs.append(b.mincut(tr, rc))
            w += b.activate(segs[1])
        rec.update(segments=segs, activated=w)
        if w == 0:                                                   # :556-563
            rec.update(Cv=self.Cv.copy(), rX=self.rX.copy(), rV=self.rV, rE=self.rE,
                       reduced=None, preAt=None, pfdr_it=None, active=b.active(),
                       dif=real(0) if self.track else None)
            return rec
        Cv, Vc, rVc = b.components()                                 # :568-597
        rV = rVc.size - 1
        rEu, rEv, rLa, rL1 = b.reduced_graph(float(self.eps))        # :599-661
        pit = self.PFDR_it
        preAt = N <= 0 or rV < (2 * N * pit) // (N + pit)            # :671
        red = b.reduce(N, self.A, self.Y, preAt)                     # :672-836
        if preAt:                                                    # :848-859
            n = 0 if N == 0 else -rV
            pY, pA = red["rY"], red["rAA"]
        else:
            n = N
            pY, pA = self.Y, np.ascontiguousarray(red["rA"].T)       # column rv contiguous
        rX, self.PFDR_it = b.pfdr(n, pY, pA, rEu, rEv, rLa, rL1, self.positivity, red["L"],
                                  **self.par)
        rX = np.ascontiguousarray(rX, self.dt)
        b.set_values(rX)
        b.merge(float(self.eps), float(self.CP_difTol))              # :863-886
        if N > 0:                                                    # :889-901
            a = np.zeros(N, self.dt)
            rA = red["rA"]
            for rv in range(rV):
                a = a + rA[:, rv] * rX[rv]
            self.R = self.Y - a
        dif = None
        if self.track:                                               # :905-923
            Cv_, rX_ = self._last
            xa = rX[Cv]
            d = rX_[Cv_] - xa
            dif = seq_sum(d * d)
            c = seq_sum(xa * xa)
            dif = dif / c if c > self.eps else dif / self.eps
            self._last = (Cv.copy(), rX.copy())
        self.Cv, self.rX, self.rV, self.rE = Cv.copy(), rX, rV, rEu.size
        rec.update(Cv=self.Cv.copy(), rX=rX.copy(), rV=rV, rE=rEu.size, Vc=Vc.copy(),
                   rVc=rVc.copy(), reduced=dict(rEu=rEu, rEv=rEv, rLa_d1=rLa, rLa_l1=rL1,
                                                rY=red["rY"], rAA=red["rAA"], L=red["L"]),
                   preAt=bool(preAt), pfdr_it=self.PFDR_it, active=b.active(), dif=dif)
        return rec

    # ------------------------------------------------------ the main loop --
    def run(self, CP_itMax):
        """from the initial state -> (rX0, [one record per iteration]); the
        loop ends like the reference's (:335): CP_it == CP_itMax or dif < CP_difTol^2"""
        real = self.dt.type
        rX0 = self.initialize().copy()
        dif = self.difTol2 if self.difTol2 > real(1) else real(1)    # :313
        recs = []
        while not (len(recs) == CP_itMax or dif < self.difTol2):     # :335
            rec = self.iterate()
            if self.track:
                dif = rec["dif"]
            recs.append(rec)
        return rX0, recs


def gpu_twin(p, track=True, **over):
    """the twin over the library's steps for a cp_problems.problem() dict, of
    the dict's flavour (``kind``)"""
    q = dict(p)
    q.update(over)
    b = GpuBackend(q["V"], q["Eu"], q["Ev"], q["La_d1"], q["La_l1"], q["kind"],
                   q.get("lo", -np.inf), q.get("hi", np.inf))
    t = Twin(b, q["V"], q["N"], q["Y"], q["A"], positivity=q["positivity"],
             CP_difTol=q["CP_difTol"], rho=q["rho"], condMin=q["condMin"], difRcd=q["difRcd"],
             difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"], La_l1=q["La_l1"], track=track)
    return t


def canonical(Cv):
    """component labels renumbered by first appearance"""
    Cv = np.asarray(Cv)
    _, first, inv = np.unique(Cv, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))
    return order[inv]
