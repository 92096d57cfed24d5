"""Cut pursuit with the reduced operator kept sparse, on the GPU
(pfdr_cp_reduce_csc_sparse_*, pfdr_cp_solver_set_reduced).

The sparse rA, l and the residual owe the dense code's bytes (the skipped terms
are +-0 added to sums that started at +0); L and the reduced solve follow the
CSC power method and a sparse session, so the solver owes the bytes of the same
steps composed through the public entries (cp_reduced_sparse.SparseBackend
under cp_twin.Twin), and the dense mode's results within a measured gap."""
import functools

import numpy as np
import pytest

import cp_reduced_sparse as RS
import cp_sparse_cases as SC
from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import uniform

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTS = pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
same = SC.same_bytes


# ------------------------------------------------------------- 1. reduce --
def _partition(name, V):
    if name == "identity":  # rV = V, every vertex its own component, in order
        return np.arange(V + 1, dtype=np.int32), np.arange(V, dtype=np.int32)
    return SC.partition(name, V)


REDUCE = [(m, q) for m in SC.MATRICES for q in SC.PARTITIONS + ("identity",)
          if _partition(q, SC.matrix(m)[0].shape[1]) is not None]
_l_rel = {}  # case -> the largest relative difference of L against the dense entry's


@functools.lru_cache(maxsize=None)
def _reduce(mat, part, dt):
    """-> (csc, rVc, Vc, the sparse step's result, the dense entry's on the same CSC)"""
    N, V = SC.matrix(mat)[0].shape
    c = SC.csc(mat, dt)
    rVc, Vc = _partition(part, V)
    Y = (2 * uniform(91, np.arange(N, dtype=np.uint64)) - 1).astype(dt)
    got = pfdr.cp_reduce(N, c, Y, rVc, Vc, preAt=False, reduced="sparse")
    ref = pfdr.cp_reduce(N, c, Y, rVc, Vc, preAt=False)
    return c, rVc, Vc, got, ref


@DTS
@pytest.mark.parametrize("mat,part", REDUCE, ids=["%s-%s" % r for r in REDUCE])
def test_reduce_keeps_the_dense_bytes_in_a_csc(gpu_lib, mat, part, dt):
    c, rVc, Vc, got, ref = _reduce(mat, part, dt)
    rA, N, rV = got["rA"], c.N, rVc.size - 1
    assert isinstance(rA, pfdr.CSC) and rA.shape == (N, rV) and rA.dtype == np.dtype(dt)
    assert got["rAA"] is None and got["rY"] is None
    # well formed, rows strictly ascending inside a column
    assert rA.colptr[0] == 0 and rA.colptr[-1] == rA.nnz <= c.nnz
    assert np.all(np.diff(rA.colptr) >= 0)
    assert rA.rowidx.size == rA.nnz and np.all((0 <= rA.rowidx) & (rA.rowidx < N))
    cols = np.repeat(np.arange(rV), np.diff(rA.colptr))
    inside = cols[1:] == cols[:-1]
    assert np.all(np.diff(rA.rowidx.astype(np.int64))[inside] > 0)
    # the structure: some stored A[n, v] with v in component rv
    st = np.zeros((N, rV), bool)
    st[rA.rowidx, cols] = True
    assert np.array_equal(st, RS.stored_model(c, rVc, Vc))
    # the values and l: the dense entry's bytes
    assert same(rA.to_dense(), ref["rA"]), np.argwhere(rA.to_dense() != ref["rA"])[:5]
    assert same(got["Leq"], ref["Leq"])
    # L = l (l c) as k_cp_lipschitz rounds it (x = l; x *= l * c), c from the
    # public CSC power method on the scaled entries
    l = got["Leq"]
    scaled = pfdr.CSC(rA.colptr, rA.rowidx, rA.val / l[cols], N)
    assert scaled.dtype == np.dtype(dt)
    cn = dt(pfdr.operator_norm(scaled, 1e-3, 100, 10)[0])
    want = l * (l * cn)
    assert same(got["L"], want), (cn, np.flatnonzero(got["L"] != want)[:5])


# -------------------------------------- 2. L against the dense cp_reduce --
@DTS
def test_L_is_close_to_the_dense_entrys(gpu_lib, dt):
    """two power-method estimates of c at nTol 1e-3 (the dense entry takes its
    Gram branch at these sizes): ten times the measured difference, 1e-2 at most"""
    worst = 0.0
    for mat, part in REDUCE:
        _, _, _, got, ref = _reduce(mat, part, dt)
        rel = float(np.max(np.abs(got["L"].astype(F64) - ref["L"].astype(F64)) /
                           np.abs(ref["L"].astype(F64))))
        _l_rel[(mat, part, np.dtype(dt).name)] = rel
        worst = max(worst, rel)
    where = max(_l_rel, key=_l_rel.get)
    print("L sparse vs dense, largest relative difference (%s): %.3e at %s" % (
        np.dtype(dt).name, worst, where))
    assert worst <= RS.bound(RS.L_REL_MEASURED, 1e-2), (worst, where)


# ------------------------------------------------ 3. residual and restart --
@DTS
@pytest.mark.parametrize("mat", ["r300", "blur"])
def test_a_recomputed_residual_has_the_dense_modes_bytes(gpu_lib, mat, dt):
    p = RS.problem(mat, dt)
    V, Eu, Ev = p["V"], p["Eu"], p["Ev"]
    sp, de = RS.solver(p, "l1", "sparse"), RS.solver(p, "l1")
    for part in ("one_perm", "bands", "singletons"):
        rVc, Vc = SC.partition(part, V)
        Cv = SC.cv_of(rVc, Vc)
        rX = (2 * uniform(97, np.arange(rVc.size - 1, dtype=np.uint64)) - 1).astype(dt)
        state = dict(Cv=Cv, Vc=Vc, rVc=rVc, rX=rX, active=(Cv[Eu] != Cv[Ev]).astype(np.uint8))
        for s in (sp, de):
            s.set_state(state, R=None)
        got, ref = sp.state(), de.state()
        assert same(got["R"], ref["R"]), (part, np.flatnonzero(got["R"] != ref["R"])[:5])
        assert np.all(np.isfinite(got["R"])) and np.any(got["R"] != p["Y"])
        lab = Cv
        for s in (sp, de):
            s.set_partition(lab, rX)
        assert same(sp.state()["R"], de.state()["R"]), (part, "set_partition")
    sp.close()
    de.close()


# ---------------------------------------- 4. solver against the step twin --
@functools.lru_cache(maxsize=None)
def _twin_run(name, flavour, dt):
    """-> (rX0, records, (sparse iterations, dense direct iterations, max rnnz))"""
    p = RS.problem(name, dt)
    t = RS.twin(p, flavour)
    rX0, recs = t.run(8)
    counts = (t.b.sparse_its, t.b.dense_direct_its, t.b.max_rnnz)
    t.b.close()
    return rX0, recs, counts


def _check_against_twin(p, run, rX0, recs, k, what):
    Cv, rX, it, Obj, Dif, _ = run
    assert it == min(k, len(recs)), (what, it, len(recs))
    if it == 0:
        assert not Cv.any() and same(rX, rX0), what
        return
    r = recs[it - 1]
    assert same(Cv, r["Cv"]), (what, "Cv")
    assert same(rX, r["rX"]), (what, "rX", np.flatnonzero(rX != r["rX"])[:5])
    want = np.array([x["dif"] for x in recs[:it]], rX.dtype)
    assert same(Dif[:it], want), (what, "Dif", Dif[:it], want)


@DTS
@pytest.mark.parametrize("flavour", list(RS.FLAVOURS))
@pytest.mark.parametrize("name", RS.PROBLEMS)
def test_solver_is_the_step_twin(gpu_lib, name, flavour, dt):
    p = RS.problem(name, dt)
    rX0, recs, counts = _twin_run(name, flavour, dt)
    direct = [r["preAt"] is False for r in recs]
    print(name, flavour, np.dtype(dt).name, "rV", [r["rV"] for r in recs], "direct", direct,
          "twin counts", counts)
    if name.startswith("direct12"):  # N = 12: the threshold lies below 24 for any pit
        assert any(direct), "no direct iteration"
    for k in (0, 1, 2, 8):
        s = RS.solver(p, flavour, "sparse")
        run = s.run(**RS.params(p, CP_itMax=k))
        _check_against_twin(p, run, rX0, recs, k, (name, flavour, k))
        stats = s.reduced_stats()
        s.close()
        n = sum(direct[:run[2]])
        assert stats[0] == n and stats[1] == 0, (k, stats, n)
        assert (stats[2] > 0) == (n > 0) and stats[2] <= p["csc"].nnz
    assert stats == counts, (stats, counts)  # the whole run's


@DTS
@pytest.mark.parametrize("name,flavour", [("direct12_thin", "l1"), ("direct12_thin", "bounds"),
                                          ("blur", "duplex")])
def test_device_inputs_and_fresh_solvers_give_the_same_bytes(gpu_lib, name, flavour, dt):
    p = RS.problem(name, dt)
    q = RS.params(p)
    runs = []
    for device in (False, False, True):
        s = RS.solver(p, flavour, "sparse", device=device)
        runs.append((s.run(**q), s.state()["R"], s.reduced_stats()))
        s.close()
    for other in runs[1:]:
        for k in (0, 1, 3, 4):
            assert same(other[0][k], runs[0][0][k]), k
        assert other[0][2] == runs[0][0][2] and other[2] == runs[0][2]
        assert same(other[1], runs[0][1])


def test_the_mode_can_change_between_runs(gpu_lib):
    """one iteration in the dense mode, one in the sparse mode from the state
    that is kept, and back: a dense-mode iteration from a dense solver's state"""
    p = RS.problem("direct12_thin", F32)
    a, b = RS.solver(p, "l1"), RS.solver(p, "l1")
    q = RS.params(p, CP_itMax=1)
    ra, rb = a.run(**q), b.run(**q)
    assert same(ra[1], rb[1]) and a.reduced_stats() == b.reduced_stats() == (0, 1, 0)
    before = b.state()
    b.set_reduced("sparse")
    after = b.state()
    assert all(same(before[k], after[k]) for k in before)
    a.run(**q)
    b.run(**q)
    assert a.reduced_stats() == (0, 1, 0) and b.reduced_stats()[:2] == (1, 0)
    assert b.reduced_stats()[2] > 0
    b.set_reduced("dense")
    b.set_state(a.state())
    ra, rb = a.run(**q), b.run(**q)
    assert same(ra[0], rb[0]) and same(ra[1], rb[1]) and b.reduced_stats() == a.reduced_stats()
    assert b.reduced_stats()[0] == 0
    a.close()
    b.close()


# ---------------------------------------------------------- 5. zero column --
@DTS
def test_a_zero_column_of_its_own_is_refused_by_the_step(gpu_lib, dt):
    A, st = RS.zero_column_matrix(dt)
    c = pfdr.CSC.from_dense(A, st)
    N, V = A.shape
    Y = np.ones(N, dt)
    rVc, Vc = SC.partition("singletons", V)  # vertex v is component V - 1 - v
    rv = V - 1 - RS.ZERO_AT
    with pytest.raises(pfdr.PFDRError, match=r"reduced column %d %s" % (rv, RS.ZERO_NORM)):
        pfdr.cp_reduce(N, c, Y, rVc, Vc, preAt=False, reduced="sparse")
    # in a component with a neighbour the column is accepted
    rVc2 = np.delete(rVc, rv + 1)
    got = pfdr.cp_reduce(N, c, Y, rVc2, Vc, preAt=False, reduced="sparse")
    assert same(got["rA"].to_dense(), pfdr.cp_reduce(N, c, Y, rVc2, Vc, preAt=False)["rA"])


@DTS
def test_a_zero_column_falls_back_to_the_dense_branch(gpu_lib, dt):
    """Vertex 17 is isolated and its column is zero: it is a component of its
    own from the first cut on, every iteration is direct (N = 2), and the sparse
    mode takes the dense direct branch, as the twin's reduce does.  That branch
    divides the column by its norm 0, as the reference does: from there on the
    run carries NaN in the dense mode too, and the next cut refuses NaN
    capacities.  So the run to CP_itMax = 4 ends the same way in the solver and
    in the twin -- the same bytes, or both refused -- and the run to
    CP_itMax = 1, which ends before that cut, is compared byte for byte."""
    p = RS.problem("zero_column", dt)
    outcome = []
    for k in (1, 4):
        t = RS.twin(p, "l1")
        s = RS.solver(p, "l1", "sparse")
        try:
            rX0, recs = t.run(k)
            twin_err = None
        except pfdr.PFDRError as e:
            twin_err = str(e)
        try:
            run = s.run(**RS.params(p, CP_itMax=k))
            err = None
        except pfdr.PFDRError as e:
            err = str(e)
        stats = s.reduced_stats()
        counts = (t.b.sparse_its, t.b.dense_direct_its, t.b.max_rnnz)
        s.close()
        t.b.close()
        outcome.append((k, err, twin_err, stats, counts))
        print("zero column, CP_itMax", k, "solver:", err, "| twin:", twin_err, "| stats", stats,
              "twin", counts)
        assert (err is None) == (twin_err is None), (k, err, twin_err)
        assert stats == counts, (k, stats, counts)
        assert stats[1] >= 1 and stats[0] == 0, stats  # the fallbacks, counted as dense
        if err is None:
            Cv, rX, it, _, Dif, _ = run
            assert it == len(recs) and same(Cv, recs[-1]["Cv"]) and same(rX, recs[-1]["rX"])
        else:
            assert "NaN" in err and "NaN" in twin_err, (err, twin_err)
    assert outcome[0][1] is None, "the run to CP_itMax = 1 ends before any NaN reaches a cut"


# ------------------------------------------------- 6. against the dense mode --
@DTS
def test_the_functional_is_the_dense_modes_within_the_measured_gap(gpu_lib, dt):
    """the yardstick is the dense mode, pinned to the reference's recorded runs;
    the two modes differ in the estimate of c only"""
    worst, where = 0.0, None
    for name in RS.PROBLEMS:
        p = RS.problem(name, dt)
        for flavour in RS.FLAVOURS:
            F = []
            for mode in ("sparse", "dense"):
                s = RS.solver(p, flavour, mode)
                Cv, rX = s.run(**RS.params(p))[:2]
                s.close()
                F.append(RS.functional(p, flavour, Cv, rX))
            gap = abs(F[0] - F[1]) / abs(F[1])
            print("functional, sparse vs dense mode: %-14s %-7s %s %.17g %.17g gap %.3e" % (
                name, flavour, np.dtype(dt).name, F[0], F[1], gap))
            if gap > worst:
                worst, where = gap, (name, flavour)
    print("largest relative gap (%s): %.3e at %s" % (np.dtype(dt).name, worst, where))
    assert worst <= RS.bound(RS.OBJ_GAP_MEASURED), (worst, where)


# ------------------------------------------------------------- 7. refusals --
def test_refusals(gpu_lib):
    p = RS.problem("r300", F32)
    dense = RS.solver(p, "l1", dense_A=True)
    with pytest.raises(pfdr.PFDRError, match="pfdr_cp_solver_set_reduced.*create_sparse"):
        dense.set_reduced("sparse")
    dense.close()
    with pytest.raises(pfdr.PFDRError, match="create_sparse"):
        RS.solver(p, "l1", "sparse", dense_A=True)
    Q = np.full((p["V"], 3), 1 / 3, F32)
    simplex = pfdr.CPSolver("simplex", Q.ravel(), p["Eu"], p["Ev"], p["La_d1"], K=3)
    with pytest.raises(pfdr.PFDRError, match="pfdr_cp_solver_set_reduced.*simplex"):
        simplex.set_reduced("sparse")
    simplex.close()
    s = RS.solver(p, "l1")
    with pytest.raises(pfdr.PFDRError, match="pfdr_cp_solver_set_reduced.*mode"):
        s.set_reduced(7)
    with pytest.raises(ValueError):
        s.set_reduced("sparser")
    s.set_reduced("sparse")
    s.set_reduced("dense")
    s.close()
    rVc, Vc = SC.partition("bands", p["V"])
    with pytest.raises(ValueError, match="preAt"):
        pfdr.cp_reduce(p["N"], p["csc"], p["Y"], rVc, Vc, preAt=True, reduced="sparse")
    with pytest.raises(ValueError, match="CSC"):
        pfdr.cp_reduce(p["N"], p["A"], p["Y"], rVc, Vc, preAt=False, reduced="sparse")
    for fn, args in ((pfdr.CP_quadratic_l1, (p["La_l1"],)),
                     (pfdr.CP_quadratic_l1_duplex, (p["La_l1"],))):
        with pytest.raises(ValueError, match="CSC"):
            fn(p["Y"], p["Eu"], p["Ev"], p["La_d1"], p["A"], *args, reduced="sparse")
    tail = (1e-4, 2, 1.5, 1e-3, 0.0, 1e-5, 500)
    with pytest.raises(ValueError, match="CSC"):
        pfdr.CP_PFDR_graph_quadratic_d1_bounds(p["Y"], p["A"], p["Eu"], p["Ev"], p["La_d1"],
                                               (-0.3, 0.8), *tail, reduced="sparse")
    with pytest.raises(ValueError, match="CSC"):
        pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex(p["Y"], p["A"], p["Eu"], p["Ev"], p["La_d1"],
                                                  p["La_l1"], 0, *tail, reduced="sparse")


# ----------------------------------------------------------- 8. front ends --
def test_the_front_ends_pass_the_mode_through(gpu_lib):
    p = RS.problem("direct12_thin", F32)
    q = RS.params(p)
    s = RS.solver(p, "duplex", "sparse")
    want = s.run(**q)
    assert s.reduced_stats()[0] > 0
    s.close()
    tail = (q["CP_difTol"], q["CP_itMax"], q["rho"], q["condMin"], q["difRcd"], q["difTol"],
            q["itMax"])
    got = pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex(p["Y"], p["csc"], p["Eu"], p["Ev"],
                                                    p["La_d1"], p["La_l1"], 0, *tail,
                                                    reduced="sparse")
    assert same(got[0], want[0]) and same(got[1], want[1])
    got = pfdr.CP_quadratic_l1_duplex(p["Y"], p["Eu"], p["Ev"], p["La_d1"], p["csc"], p["La_l1"],
                                      0, q["rho"], q["condMin"], q["CP_difTol"], q["difRcd"],
                                      q["difTol"], q["CP_itMax"], q["itMax"], reduced="sparse")
    assert same(got[0], want[0].astype(np.uint32)) and same(got[1], want[1])
    s = RS.solver(p, "bounds", "sparse")
    want = s.run(**q)
    s.close()
    got = pfdr.CP_PFDR_graph_quadratic_d1_bounds(p["Y"], p["csc"], p["Eu"], p["Ev"], p["La_d1"],
                                                 (RS.BOX["lo"], RS.BOX["hi"]), *tail,
                                                 reduced="sparse")
    assert same(got[0], want[0]) and same(got[1], want[1])
    s = RS.solver(p, "l1", "sparse")
    want = s.run(**q)
    s.close()
    got = pfdr.CP_quadratic_l1(p["Y"], p["Eu"], p["Ev"], p["La_d1"], p["csc"], p["La_l1"], 0,
                               q["rho"], q["condMin"], q["CP_difTol"], q["difRcd"], q["difTol"],
                               q["CP_itMax"], q["itMax"], reduced="sparse")
    assert same(got[0], want[0].astype(np.uint32)) and same(got[1], want[1])
