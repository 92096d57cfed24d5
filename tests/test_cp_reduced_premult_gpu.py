"""Premultiplied cut-pursuit iterations on the stored entries of a sparse rA, on
the GPU (pfdr_cp_reduce_csc_sparse_preAt_*, PFDR_REDUCED_SPARSE_ALL,
pfdr_cp_solver_premultiplied_stats).

rAA = rA^t rA and rY = rA^t Y summed over the stored common rows leave out only
+-0 terms of sums that started at +0 (tests/test_cp_reduced_premult_cpu.py
models it), and everything downstream is the dense code on rAA.  So the
reference of every check here is the library's own dense path on the same CSC,
byte for byte: the step, the solver's runs, its states and records."""
import ctypes as C
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
WINDOW = "PFDR_CP_GRAM_WINDOW"  # read by the library at every call
ERR_ARG = 1


# --------------------------------------------------------------- 1. step --
def _partition(name, V):
    if name == "identity":  # rV = V, every vertex its own component, in order
        return np.arange(V + 1, dtype=np.int32), np.arange(V, dtype=np.int32)
    return SC.partition(name, V)


STEP = [(m, q) for m in SC.MATRICES for q in SC.PARTITIONS + ("identity",)
        if _partition(q, SC.matrix(m)[0].shape[1]) is not None]


def _observation(N, dt):
    return (2 * uniform(91, np.arange(N, dtype=np.uint64)) - 1).astype(dt)


@functools.lru_cache(maxsize=None)
def _dense_step(mat, part, dt):
    """-> (csc, rVc, Vc, Y, the dense entry's premultiplied result on the CSC)"""
    N, V = SC.matrix(mat)[0].shape
    c = SC.csc(mat, dt)
    rVc, Vc = _partition(part, V)
    Y = _observation(N, dt)
    ref = pfdr.cp_reduce(N, c, Y, rVc, Vc, preAt=True)
    again = pfdr.cp_reduce(N, c, Y, rVc, Vc, preAt=True)
    assert same(ref["L"], again["L"]), "the dense entry: fixed starts, no atomics"
    return c, rVc, Vc, Y, ref


def _sparse_step(c, Y, rVc, Vc):
    return pfdr.cp_reduce(c.N, c, Y, rVc, Vc, preAt=True, reduced="sparse_all")


def _check_step(c, rVc, Vc, got, ref, what):
    rA, N, rV = got["rA"], c.N, rVc.size - 1
    for k in ("rAA", "rY", "Leq", "L"):
        assert same(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5])
    assert got["rAA"].shape == (rV, rV) and np.all(np.isfinite(got["L"]))
    assert isinstance(rA, pfdr.CSC) and rA.shape == (N, rV) and rA.dtype == c.dtype
    assert same(rA.to_dense(), ref["rA"]), (what, np.argwhere(rA.to_dense() != ref["rA"])[:5])
    # well formed: rows strictly ascending inside a column, the structure of the model
    assert rA.colptr[0] == 0 and rA.colptr[-1] == rA.nnz <= c.nnz
    assert np.all(np.diff(rA.colptr) >= 0)
    assert rA.rowidx.size == rA.nnz and np.all((0 <= rA.rowidx) & (rA.rowidx < N))
    cols = np.repeat(np.arange(rV), np.diff(rA.colptr))
    inside = cols[1:] == cols[:-1]
    assert np.all(np.diff(rA.rowidx.astype(np.int64))[inside] > 0), what
    st = np.zeros((N, rV), bool)
    st[rA.rowidx, cols] = True
    assert np.array_equal(st, RS.stored_model(c, rVc, Vc)), what


@DTS
@pytest.mark.parametrize("mat,part", STEP, ids=["%s-%s" % r for r in STEP])
def test_step_has_the_dense_entrys_bytes(gpu_lib, mat, part, dt, monkeypatch):
    monkeypatch.delenv(WINDOW, raising=False)
    c, rVc, Vc, Y, ref = _dense_step(mat, part, dt)
    _check_step(c, rVc, Vc, _sparse_step(c, Y, rVc, Vc), ref, (mat, part))


# ------------------------------------------------------------ 2. windows --
WINDOWED = [r for r in STEP if r[0] in ("r300", "blur", "longrun")]


@DTS
@pytest.mark.parametrize("window", [64, 1])
@pytest.mark.parametrize("mat,part", WINDOWED, ids=["%s-%s" % r for r in WINDOWED])
def test_the_window_changes_no_byte(gpu_lib, mat, part, window, dt, monkeypatch):
    """N = 200, 480 and 40 rows: several windows of 64 rows (one for "longrun"),
    and a window per row"""
    c, rVc, Vc, Y, ref = _dense_step(mat, part, dt)
    monkeypatch.delenv(WINDOW, raising=False)
    default = _sparse_step(c, Y, rVc, Vc)
    monkeypatch.setenv(WINDOW, str(window))
    got = _sparse_step(c, Y, rVc, Vc)
    for k in ("rAA", "rY", "Leq", "L"):
        assert same(got[k], default[k]) and same(got[k], ref[k]), (mat, part, window, k)
    assert same(got["rA"].val, default["rA"].val)


# --------------------------------------------- 3. tall, the default window --
TALL_N, TALL_V, TALL_SINGLE = 40009, 96, 5


@functools.lru_cache(maxsize=None)
def _tall():
    """2 % fill; the last row fully stored; column 5 stores its entry of that
    row only.  160 KB of f32 rows: several windows at any window that fits LDS"""
    A, st = (a.copy() for a in SC._random_fill(31, TALL_N, TALL_V, 0.02))
    A[:, TALL_SINGLE], st[:, TALL_SINGLE] = 0.0, False
    last = 2.0 * uniform(32, np.arange(TALL_V, dtype=np.uint64)) - 1.0
    last[last == 0] = 0.5
    A[TALL_N - 1], st[TALL_N - 1] = last, True
    assert st[:, TALL_SINGLE].sum() == 1 and st[TALL_N - 1].all()
    return A, st


def _tall_partition(rV):
    i = np.arange(TALL_V)
    Vc = ((7 * i + 3) % TALL_V).astype(np.int32)  # 7 is coprime to 96
    return ((TALL_V * np.arange(rV + 1)) // rV).astype(np.int32), Vc  # 13 or 14 each for rV = 7


@DTS
@pytest.mark.parametrize("rV", [1, 7, 96])
def test_tall_matrix_at_the_default_window(gpu_lib, rV, dt, monkeypatch):
    monkeypatch.delenv(WINDOW, raising=False)
    A, st = _tall()
    c = pfdr.CSC.from_dense(A.astype(dt), st)
    rVc, Vc = _tall_partition(rV)
    Y = _observation(TALL_N, dt)
    ref = pfdr.cp_reduce(TALL_N, c, Y, rVc, Vc, preAt=True)
    _check_step(c, rVc, Vc, _sparse_step(c, Y, rVc, Vc), ref, ("tall", rV))


# ------------------------------------ 4. solver, premultiplied throughout --
def _run(p, flavour, mode, device=False, **over):
    """-> (run, R of the final state, premultiplied_stats, reduced_stats)"""
    s = RS.solver(p, flavour, mode, device=device)
    try:
        run = s.run(**RS.params(p, **over))
        return run, s.state()["R"], s.premultiplied_stats(), s.reduced_stats()
    finally:
        s.close()


def _same_run(a, b, what):
    """Cv, rX, the iteration count, Obj, Dif"""
    assert a[2] == b[2], (what, a[2], b[2])
    for k, name in ((0, "Cv"), (1, "rX"), (3, "Obj"), (4, "Dif")):
        assert same(a[k], b[k]), (what, name)


@DTS
@pytest.mark.parametrize("flavour", list(RS.FLAVOURS))
@pytest.mark.parametrize("name", ["blur", "r300"])
def test_solver_premultiplied_throughout(gpu_lib, name, flavour, dt):
    """A run whose iterations are all premultiplied -- the dense solver's
    reduced_stats() is (0, 0, 0): every run of "blur", and of "r300" to
    CP_itMax 1 -- has the dense mode's bytes.  "r300" (N = 200) takes a direct
    iteration as its second, measured in every flavour and both types (2 of the
    whole run's 7 or 8 reductions are direct, the others premultiplied), in the
    dense mode too, whose reduced_stats() then cannot be (0, 0, 0); there the
    direct iterations follow the "sparse" mode (another estimate of c), so such
    a run owes the "sparse" mode's bytes, as in the mixed test below."""
    p = RS.problem(name, dt)
    for over in (dict(), dict(CP_itMax=1), dict(CP_itMax=2)):
        what = (name, flavour, over)
        got, R, pre, red = _run(p, flavour, "sparse_all", **over)
        ref, R0, pre0, red0 = _run(p, flavour, "dense", **over)
        k = pre[0]
        assert k > 0 and pre[1] == 0 and 0 < pre[2] <= p["csc"].nnz, (what, pre)
        assert k <= got[2]  # (an iteration whose cut activates nothing reduces nothing)
        if name == "blur" or over.get("CP_itMax") == 1:
            assert red0 == (0, 0, 0), (what, red0)
        print(what, np.dtype(dt).name, "CP_it", got[2], "premultiplied", pre, "dense mode",
              pre0, "direct", red, "dense mode", red0)
        if red0 == (0, 0, 0):  # premultiplied throughout
            _same_run(got, ref, what)
            assert same(R, R0), what
            assert pre0 == (0, k, 0), (what, pre0)
            assert red == (0, 0, 0), (what, red)
        else:
            ref, R0, pre0, red0 = _run(p, flavour, "sparse", **over)
            _same_run(got, ref, what)
            assert same(R, R0), what
            assert pre0 == (0, k, 0) and red == red0, (what, pre0, red, red0)


# ------------------------------------------------------ 5. solver, mixed --
@DTS
@pytest.mark.parametrize("flavour", list(RS.FLAVOURS))
@pytest.mark.parametrize("name", ["direct12", "direct12_thin"])
def test_solver_mixed_iterations(gpu_lib, name, flavour, dt):
    p = RS.problem(name, dt)
    got, R, pre, red = _run(p, flavour, "sparse_all")
    ref, R0, pre0, red0 = _run(p, flavour, "sparse")
    _same_run(got, ref, (name, flavour))
    assert same(R, R0)
    assert red == red0 and red[0] > 0, (red, red0)
    assert pre0[0] == 0 and pre0[2] == 0 and pre[:2] == (pre0[1], 0), (pre, pre0)
    assert (pre[2] > 0) == (pre[0] > 0) and pre[2] <= p["csc"].nnz


# ------------------------------------------------------ 6. between runs --
def test_the_mode_can_change_between_runs(gpu_lib):
    p = RS.problem("blur", F32)
    a, b = RS.solver(p, "l1"), RS.solver(p, "l1")
    q = RS.params(p, CP_itMax=1)
    ra, rb = a.run(**q), b.run(**q)
    _same_run(ra, rb, "first")
    assert a.premultiplied_stats() == b.premultiplied_stats() == (0, 1, 0)
    before = b.state()
    b.set_reduced("sparse_all")
    after = b.state()
    assert all(same(before[k], after[k]) for k in before)
    ra, rb = a.run(**q), b.run(**q)
    _same_run(ra, rb, "second")
    assert same(a.state()["R"], b.state()["R"])
    assert a.premultiplied_stats() == (0, 1, 0)
    pre = b.premultiplied_stats()
    assert pre[:2] == (1, 0) and 0 < pre[2] <= p["csc"].nnz
    b.set_reduced("dense")
    ra, rb = a.run(**q), b.run(**q)
    _same_run(ra, rb, "third")
    assert b.premultiplied_stats() == a.premultiplied_stats() == (0, 1, 0)
    # a residual recomputed in mode 2: the dense mode's
    st = a.state()
    b.set_reduced("sparse_all")
    for s in (a, b):
        s.set_state(st, R=None)
    assert same(a.state()["R"], b.state()["R"])
    assert np.any(b.state()["R"] != p["Y"])
    a.close()
    b.close()


@DTS
@pytest.mark.parametrize("name,flavour", [("blur", "duplex"), ("r300", "bounds")])
def test_device_inputs_and_fresh_solvers_give_the_same_bytes(gpu_lib, name, flavour, dt):
    p = RS.problem(name, dt)
    runs = [_run(p, flavour, "sparse_all", device=device) for device in (False, False, True)]
    for other in runs[1:]:
        _same_run(other[0], runs[0][0], (name, flavour))
        assert same(other[1], runs[0][1]) and other[2:] == runs[0][2:]


# ----------------------------------------------------------- 7. refusals --
def _raw_step(lib, sfx, ct, c, Y, rVc, Vc, colptr=None, rowidx=None, drop=()):
    """the C entry on host arrays -> (status, message, rAA, rnnz); ``drop``: the
    outputs passed as NULL"""
    dt = c.dtype
    colptr = c.colptr if colptr is None else np.ascontiguousarray(colptr, np.int64)
    rowidx = c.rowidx if rowidx is None else np.ascontiguousarray(rowidx, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    st = pfdr.CSCStruct(c.nnz, colptr.ctypes.data, rowidx.ctypes.data, c.val.ctypes.data)
    rV = rVc.size - 1
    out = dict(rAA=np.zeros((rV, rV), dt), rY=np.zeros(rV, dt), rcolptr=np.zeros(rV + 1, np.int64),
               rrowidx=np.zeros(c.nnz, np.int32), rval=np.zeros(c.nnz, dt))
    rnnz = C.c_int64(-1)
    arg = lambda k: None if k in drop else p(out[k])
    status = getattr(lib, "pfdr_cp_reduce_csc_sparse_preAt_" + sfx)(
        C.c_int(c.N), C.c_int(c.V), C.byref(st), p(Y), C.c_int(rV), p(rVc), p(Vc),
        C.c_int(pfdr.PFDR_MEM_HOST), ct(1e-3), C.c_int(100), C.c_int(10), arg("rAA"), arg("rY"),
        None, None, None if "rnnz" in drop else C.byref(rnnz), arg("rcolptr"), arg("rrowidx"),
        arg("rval"))
    return status, lib.pfdr_last_error().decode(), out["rAA"], rnnz.value


@pytest.mark.parametrize("sfx,ct,dt", [("f32", C.c_float, F32), ("f64", C.c_double, F64)])
def test_the_c_entry_refuses_and_recovers(gpu_lib, sfx, ct, dt):
    lib = pfdr.load()
    c, rVc, Vc, Y, ref = _dense_step("r300", "bands", dt)
    fn = "pfdr_cp_reduce_csc_sparse_preAt_" + sfx
    down = c.colptr.copy()
    down[5] = down[4] - 1
    high = c.rowidx.copy()
    high[c.colptr[7]] = c.N
    twice = c.rowidx.copy()
    e = int(np.flatnonzero(np.diff(c.colptr) >= 2)[0])
    twice[c.colptr[e] + 1] = twice[c.colptr[e]]
    bad = [(dict(drop=("rAA",)), "rAA and rY are required"),
           (dict(drop=("rY",)), "rAA and rY are required"),
           (dict(drop=("rnnz",)), "all set or all NULL"),
           (dict(drop=("rcolptr", "rval")), "all set or all NULL"),
           (dict(colptr=down), "colptr must be non-decreasing"),
           (dict(rowidx=high), "row index outside [0, N)"),
           (dict(rowidx=twice), "strictly ascending")]
    for kw, needle in bad:
        status, msg, _, _ = _raw_step(lib, sfx, ct, c, Y, rVc, Vc, **kw)
        assert status == ERR_ARG and fn in msg and needle in msg, (kw, status, msg)
        status, msg, rAA, rnnz = _raw_step(lib, sfx, ct, c, Y, rVc, Vc)  # the next valid call
        assert status == 0 and same(rAA, ref["rAA"]) and 0 < rnnz <= c.nnz, (kw, status, msg)
    # without the four CSC outputs
    status, msg, rAA, rnnz = _raw_step(lib, sfx, ct, c, Y, rVc, Vc,
                                       drop=("rnnz", "rcolptr", "rrowidx", "rval"))
    assert status == 0 and same(rAA, ref["rAA"]) and rnnz == -1, msg


def test_refusals(gpu_lib):
    p = RS.problem("r300", F32)
    dense = RS.solver(p, "l1", dense_A=True)
    with pytest.raises(pfdr.PFDRError, match="pfdr_cp_solver_set_reduced.*create_sparse"):
        dense.set_reduced("sparse_all")
    assert dense.premultiplied_stats() == (0, 0, 0)
    dense.close()
    with pytest.raises(pfdr.PFDRError, match="create_sparse"):
        RS.solver(p, "l1", "sparse_all", dense_A=True)
    Q = np.full((p["V"], 3), 1 / 3, F32)
    simplex = pfdr.CPSolver("simplex", Q.ravel(), p["Eu"], p["Ev"], p["La_d1"], K=3)
    with pytest.raises(pfdr.PFDRError, match="pfdr_cp_solver_set_reduced.*simplex"):
        simplex.set_reduced("sparse_all")
    simplex.close()
    s = RS.solver(p, "l1")
    with pytest.raises(pfdr.PFDRError, match="pfdr_cp_solver_set_reduced.*mode"):
        s.set_reduced(3)
    s.set_reduced(2)
    s.set_reduced("sparse_all")
    s.set_reduced("dense")
    s.close()
    rVc, Vc = SC.partition("bands", p["V"])
    for preAt in (True, False):
        with pytest.raises(ValueError, match="CSC"):
            pfdr.cp_reduce(p["N"], p["A"], p["Y"], rVc, Vc, preAt=preAt, reduced="sparse_all")
    # preAt = False: what "sparse" does
    got = pfdr.cp_reduce(p["N"], p["csc"], p["Y"], rVc, Vc, preAt=False, reduced="sparse_all")
    ref = pfdr.cp_reduce(p["N"], p["csc"], p["Y"], rVc, Vc, preAt=False, reduced="sparse")
    assert got["rAA"] is None and got["rY"] is None
    assert same(got["L"], ref["L"]) and same(got["rA"].val, ref["rA"].val)
    with pytest.raises(ValueError, match="CSC"):
        pfdr.CP_quadratic_l1(p["Y"], p["Eu"], p["Ev"], p["La_d1"], p["A"], p["La_l1"],
                             reduced="sparse_all")
    tail = (1e-4, 2, 1.5, 1e-3, 0.0, 1e-5, 500)
    with pytest.raises(ValueError, match="CSC"):
        pfdr.CP_PFDR_graph_quadratic_d1_bounds(p["Y"], p["A"], p["Eu"], p["Ev"], p["La_d1"],
                                               (-0.3, 0.8), *tail, reduced="sparse_all")


# --------------------------------------------------------- 8. front ends --
def test_the_front_ends_pass_the_mode_through(gpu_lib):
    p = RS.problem("blur", F32)
    q = RS.params(p)
    want, _, pre, _ = _run(p, "l1", "sparse_all")
    assert pre[0] > 0 and pre[1] == 0
    got = pfdr.CP_quadratic_l1(p["Y"], p["Eu"], p["Ev"], p["La_d1"], p["csc"], p["La_l1"], 0,
                               q["rho"], q["condMin"], q["CP_difTol"], q["difRcd"], q["difTol"],
                               q["CP_itMax"], q["itMax"], reduced="sparse_all")
    assert same(got[0], want[0].astype(np.uint32)) and same(got[1], want[1])
    want = _run(p, "bounds", "sparse_all")[0]
    tail = (q["CP_difTol"], q["CP_itMax"], q["rho"], q["condMin"], q["difRcd"], q["difTol"],
            q["itMax"])
    got = pfdr.CP_PFDR_graph_quadratic_d1_bounds(p["Y"], p["csc"], p["Eu"], p["Ev"], p["La_d1"],
                                                 (RS.BOX["lo"], RS.BOX["hi"]), *tail,
                                                 reduced="sparse_all")
    assert same(got[0], want[0]) and same(got[1], want[1])
