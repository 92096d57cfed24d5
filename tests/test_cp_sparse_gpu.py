"""Sparse A (CSC) in cut pursuit on the GPU.  Only the component column sums
and the gradient -A^t R read the CSC, adding the stored entries in the dense
loops' order, so every result must have the bytes of the library's own dense
entry on the densified matrix: no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import cp_run_cases
import cp_sparse_cases as SC
import cp_twin as T
from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import grid_graph, uniform

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTS = pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
same = SC.same_bytes
THIN_SEED = 81


# ------------------------------------------------------------- 1. reduce --
REDUCE = [(m, q) for m in SC.MATRICES for q in SC.PARTITIONS
          if SC.partition(q, SC.matrix(m)[0].shape[1]) is not None]


@DTS
@pytest.mark.parametrize("mat,part", REDUCE, ids=["%s-%s" % r for r in REDUCE])
def test_reduce_has_the_dense_bytes(gpu_lib, mat, part, dt):
    A, _ = SC.matrix(mat)
    N, V = A.shape
    c = SC.csc(mat, dt)
    rVc, Vc = SC.partition(part, V)
    Y = (2 * uniform(91, np.arange(N, dtype=np.uint64)) - 1).astype(dt)
    for preAt in (0, 1):
        got = pfdr.cp_reduce(N, c, Y, rVc, Vc, preAt=bool(preAt))
        ref = pfdr.cp_reduce(N, A.astype(dt), Y, rVc, Vc, preAt=bool(preAt))
        for k in ("rA", "rAA", "rY", "L", "Leq"):
            assert (got[k] is None) == (ref[k] is None), (k, preAt)
            if ref[k] is not None:
                assert same(got[k], ref[k]), (k, preAt, np.flatnonzero(
                    np.ravel(got[k] != ref[k]))[:5])
    # and the model's bytes (the premultiplied call leaves rA as it was summed)
    assert preAt == 1 and same(got["rA"].T, SC.model_colsum(c, rVc, Vc))


# ----------------------------------------------------------- 2. gradient --
@DTS
@pytest.mark.parametrize("l1", [False, True], ids=["d1", "d1_l1"])
def test_gradient_has_the_dense_bytes(gpu_lib, dt, l1):
    A, _ = SC.matrix("r300")
    N, V = A.shape
    Eu, Ev = grid_graph((20, 15), 4)
    E = Eu.size
    La = (0.05 * (0.5 + uniform(92, np.arange(E, dtype=np.uint64)))).astype(dt)
    L1 = (0.01 + 0.01 * uniform(93, np.arange(V, dtype=np.uint64))).astype(dt) if l1 else None
    g = pfdr.CPGraph(V, Eu, Ev, La, L1)
    rVc, Vc = SC.partition("bands", V)
    g.set_active((uniform(94, np.arange(E, dtype=np.uint64)) < 1 / 3).astype(np.uint8))
    g.set_components(SC.cv_of(rVc, Vc), Vc, rVc)
    g.set_values(np.array([0.7, 0.0, -0.4], dt))
    R = (2 * uniform(95, np.arange(N, dtype=np.uint64)) - 1).astype(dt)
    got = g.gradient(N, SC.csc("r300", dt), None, R)
    ref = g.gradient(N, A.astype(dt), None, R)
    g.close()
    assert same(got, ref), np.flatnonzero(got != ref)[:5]


# ------------------------------------------- 3. solver against the dense --
FLAVOURS = {"l1": dict(), "l1_pos": dict(positivity=1), "duplex": dict(duplex=True),
            "bounds": dict(bounds=True)}
PROBLEMS = ("direct12", "direct12_thin", "direct160", "direct160_thin", "blur")


@functools.lru_cache(maxsize=None)
def _problem(name, dt):
    """-> cp_problems-style dict with the dense N-by-V ``A`` and its ``csc``"""
    if name == "blur":
        return SC.grid_problem("blur", dt, 24, 20)
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


def _solver(p, flavour, sparse, device=False):
    f = FLAVOURS[flavour]
    kw = dict(lo=-0.3, hi=0.8) if f.get("bounds") else dict(
        La_l1=p["La_l1"], positivity=f.get("positivity", 0), duplex=f.get("duplex", False))
    A = p["csc"] if sparse else np.asfortranarray(p["A"]).ravel(order="F")
    arrs = [p["Y"], p["Eu"], p["Ev"], p["La_d1"]]
    if device:
        import torch
        arrs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]
        A = A.to_device()
        if "La_l1" in kw:
            kw["La_l1"] = torch.from_numpy(kw["La_l1"]).cuda()
    return pfdr.CPSolver("bounds" if f.get("bounds") else "l1", *arrs, A=A, N=p["N"], **kw)


def _params(p, **over):
    q = dict(CP_difTol=p["CP_difTol"], CP_itMax=p["CP_itMax"], rho=p["rho"],
             condMin=p["condMin"], difRcd=p["difRcd"], difTol=p["PFDR_difTol"],
             itMax=p["PFDR_itMax"])
    q.update(over)
    return q


def _same_run(got, ref, s_got, s_ref, what):
    for k, nm in enumerate(("Cv", "rX", "CP_it", "Obj", "Dif")):
        if nm == "CP_it":
            assert got[k] == ref[k], (what, nm, got[k], ref[k])
        else:
            assert same(got[k], ref[k]), (what, nm)
    assert same(s_got.state()["R"], s_ref.state()["R"]), (what, "R")


@DTS
@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("name", PROBLEMS)
def test_solver_has_the_dense_solvers_bytes(gpu_lib, name, flavour, dt):
    p = _problem(name, dt)
    for itmax in (0, 1, 2, 8):
        sp, de = _solver(p, flavour, True), _solver(p, flavour, False)
        assert sp.V == p["V"] and sp.N == p["N"]
        q = _params(p, CP_itMax=itmax)
        _same_run(sp.run(**q), de.run(**q), sp, de, (name, flavour, itmax))
        sp.close()
        de.close()


def test_the_thinned_direct12_takes_both_preAt_branches(gpu_lib):
    """the step-composed twin on the densified problem: its record holds for
    the sparse run, whose bytes are the dense run's"""
    p = _problem("direct12_thin", F32)
    t = T.gpu_twin(dict(p, A=np.asfortranarray(p["A"]).ravel(order="F")))
    _, recs = t.run(p["CP_itMax"])
    t.b.close()
    taken = [r["preAt"] for r in recs if r["preAt"] is not None]
    print("thinned direct12 twin: rV", [r["rV"] for r in recs], "preAt", taken)
    assert True in taken and False in taken, taken


# -------------------------------------------------------------- 4. resume --
@DTS
def test_resumed_runs_have_the_dense_solvers_bytes(gpu_lib, dt):
    p = _problem("direct12_thin", dt)
    sp, de = _solver(p, "l1", True), _solver(p, "l1", False)
    q = _params(p, CP_itMax=2)
    first = sp.run(**q)
    _same_run(first, de.run(**q), sp, de, "first")
    for s in (sp, de):
        s.set_penalties(0.5 * p["La_d1"])
    _same_run(sp.run(**q), de.run(**q), sp, de, "after set_penalties")
    for s in (sp, de):
        s.set_partition(first[0], first[1])  # R is recomputed: the sparse column sums
    assert same(sp.state()["R"], de.state()["R"])
    _same_run(sp.run(**q), de.run(**q), sp, de, "after set_partition")
    sp.close()
    de.close()


# ------------------------------------------------------- 5. device inputs --
def test_a_device_csc_gives_the_host_runs_bytes(gpu_lib):
    p = _problem("blur", F32)
    host, dev = _solver(p, "l1", True), _solver(p, "l1", True, device=True)
    q = _params(p, CP_itMax=3)
    _same_run(dev.run(**q), host.run(**q), dev, host, "device")
    host.close()
    dev.close()


# --------------------------------------------------------- 6. refused CSCs --
def _bad(what):
    c = SC.csc("r300", F32)
    colptr, rowidx = c.colptr.copy(), c.rowidx.copy()
    if what == "colptr":
        v = int(np.flatnonzero(np.diff(colptr) > 0)[3])
        colptr[v + 1] = colptr[v] - 1
    elif what == "row":
        rowidx[7] = c.N
    else:
        v = int(np.flatnonzero(np.diff(colptr) > 1)[0])
        rowidx[colptr[v] + 1] = rowidx[colptr[v]]
    return pfdr.CSC(colptr, rowidx, c.val, c.N)


@pytest.mark.parametrize("what,needle", [("colptr", "colptr must be non-decreasing"),
                                         ("row", "row index outside"),
                                         ("order", "strictly ascending")])
def test_a_malformed_csc_is_refused_by_name(gpu_lib, what, needle):
    p = SC.grid_problem("r300", F32, 20, 15)
    c = _bad(what)
    q = pfdr.CPProblem()
    q.kind, q.dtype, q.mem = pfdr.PFDR_KIND_L1, pfdr.PFDR_F32, pfdr.PFDR_MEM_HOST
    q.V, q.E, q.N = p["V"], p["E"], p["N"]
    keep = [np.ascontiguousarray(p[k]) for k in ("Y", "Eu", "Ev", "La_d1")]
    q.Y, q.Eu, q.Ev, q.La_d1 = (a.ctypes.data for a in keep)
    s = c.struct()
    lib = pfdr.load()
    h = C.c_void_p(12345)
    st = lib.pfdr_cp_solver_create_sparse(C.byref(h), C.byref(q), C.byref(s))
    msg = lib.pfdr_last_error().decode()
    assert st == 1, (st, msg)  # PFDR_ERR_ARG
    assert needle in msg, msg
    assert h.value is None
    with pytest.raises(pfdr.PFDRError, match=needle):
        pfdr.cp_reduce(c.N, c, p["Y"], *SC.partition("bands", c.V))


# ---------------------------------------------------------- 7. front ends --
@DTS
def test_the_front_ends_take_a_csc(gpu_lib, dt):
    p = SC.grid_problem("r300", dt, 20, 15)
    A, c = p["A"], p["csc"]
    for fn in (pfdr.CP_quadratic_l1, pfdr.CP_quadratic_l1_duplex):
        for pos in (0, 1):
            kw = dict(positivity=pos, CP_itMax=4, PFDR_itMax=2000)
            got = fn(p["Y"], p["Eu"], p["Ev"], p["La_d1"], c, p["La_l1"], **kw)
            ref = fn(p["Y"], p["Eu"], p["Ev"], p["La_d1"], A, p["La_l1"], **kw)
            assert same(got[0], ref[0]) and same(got[1], ref[1]), (fn.__name__, pos)
    tail = (1e-4, 4, 1.5, 1e-3, 0.0, 1e-5, 2000)
    mex = [(pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex, (p["La_l1"], 1)),
           (pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex, (0.02, 0)),
           (pfdr.CP_PFDR_graph_quadratic_d1_bounds, ((-0.3, 0.8),))]
    for fn, own in mex:
        call = lambda M: fn(p["Y"], M, p["Eu"], p["Ev"], p["La_d1"], *own, *tail, obj=True,
                            dif=True, time=True)
        got, ref = call(c), call(A)
        assert got[2] == ref[2], fn.__name__
        for k in (0, 1, 4, 5):
            assert same(got[k], ref[k]), (fn.__name__, k)
        assert got[3].shape == ref[3].shape
        quiet = fn(p["Y"], c, p["Eu"], p["Ev"], p["La_d1"], *own, *tail)
        assert quiet[3] is None and quiet[4] is None and quiet[5] is None
