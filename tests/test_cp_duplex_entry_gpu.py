"""The duplex driver's one-call cut pursuit (pfdr_cp_quadratic_d1_l1_duplex,
csrc/pfdr_cutpursuit.hip) pinned on every path of its loop.

a. N = 0: Cv, rX and CP_it equal the reference's recorded iterations
   (tests/golden/cp_duplex_*.npz) bit for bit, for every truncation
   CP_itMax = 1..6.
b. Entry against the step-composed twin (tests/cp_duplex_twin.py over the
   library's own per-step API): Cv, rX, CP_it byte-identical for every
   truncation CP_itMax = 0..K.
c. Against the reference's own recorded run (tests/golden/cp_duplex_run/):
   exact for N = 0, a two-sided bound on the functional otherwise.
d. The differentiable case: the bytes of pfdr_cp_quadratic_d1_l1.
e. Obj[k] and Dif[k] at every iteration against f64, within the derived
   bounds of test_cut_pursuit_paths_gpu.py.
f. Optional outputs, argument errors, repeatability, the stats and the front
   ends' conventions.
"""
import ctypes as C

import numpy as np
import pytest

import cp_duplex_run_cases as RC
import cp_duplex_twin as DT
import cp_problems as P
from cp_pfdr_graph_d1_amd import pfdr
from test_cp_graph_oracle import DNAMES, load_case
from test_cut_pursuit_gpu import functional
from test_cut_pursuit_paths_gpu import REL, STEP, check_obj_dif, relabel_differences, same_bytes
from test_mincut_duplex_gpu import TIES

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _args(q, CP_itMax):
    return ((q["V"], q["N"], q["Y"], q["A"], q["Eu"], q["Ev"], q["La_d1"], q["La_l1"]),
            dict(positivity=q["positivity"], CP_difTol=q["CP_difTol"],
                 CP_itMax=q["CP_itMax"] if CP_itMax is None else CP_itMax, rho=q["rho"],
                 condMin=q["condMin"], difRcd=q["difRcd"], difTol=q["PFDR_difTol"],
                 itMax=q["PFDR_itMax"]))


def entry(p, CP_itMax=None, **over):
    q = dict(p)
    q.update(over)
    a, kw = _args(q, CP_itMax)
    return pfdr.Lib().cp_quadratic_d1_l1_duplex(*a, **kw)


def l1_entry(p, CP_itMax=None):
    a, kw = _args(p, CP_itMax)
    return pfdr.Lib().cp_quadratic_d1_l1(*a, **kw)


def fixture_problem(c):
    """an iteration fixture's inputs as a cp_problems dict"""
    dt = c["Y"].dtype.type
    return dict(kind="duplex", V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=dt, CP_itMax=6,
                PFDR_itMax=STEP["itMax"], positivity=c["positivity"], CP_difTol=c["CP_difTol"],
                PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
                difRcd=STEP["difRcd"], Y=c["Y"], A=c["A"], Eu=c["Eu"], Ev=c["Ev"],
                La_d1=c["La_d1"], La_l1=c["La_l1"])


# ------------------------------------------ a. exact against the reference --
_exact = {}


@pytest.mark.parametrize("name", DNAMES)
def test_entry_is_the_reference_run(gpu_lib, name):
    """N = 0: every cut returns the reference's segments, PFDR is bit-exact in
    the graph modes and L is rAA itself, so the entry owes the reference's Cv,
    rX and CP_it exactly.  tests/test_cp_duplex_twin_cpu.py checks that the
    recorded chain is the reference's one-call run.  From the iteration of a cut
    listed in TIES on (none today), the truncations are compared with the twin."""
    c, d = load_case(name)
    p = fixture_problem(c)
    tol2 = c["Y"].dtype.type(c["CP_difTol"]) ** 2
    tie = min([k for n, k in TIES if n == name], default=None)
    recs = None
    if tie is not None:
        t = DT.gpu_twin(p)
        _, recs = t.run(p["CP_itMax"])
        t.b.close()
        print(name, "cut %d is a tie between minimum cuts: truncations from CP_itMax = %d on "
              "are compared with the twin, not with the recording" % (tie, tie + 1))
    n = 0
    for k in range(1, int(d["meta_steps"]) + 1):
        Cv, rX, it, Obj, Dif, Time = entry(p, CP_itMax=k)
        assert 1 <= it <= k
        assert it == k or Dif[it - 1] < tol2, (k, it, Dif[:it])
        if tie is not None and it - 1 >= tie:
            assert same_bytes(Cv, recs[it - 1]["Cv"]) and same_bytes(rX, recs[it - 1]["rX"])
            continue
        assert np.array_equal(Cv, d["k%d_out_Cv" % (it - 1)]), (k, it)
        want = d["k%d_out_rX" % (it - 1)]
        assert rX.dtype == want.dtype and np.array_equal(rX, want), (k, it)
        n += 1
    _exact[name] = n
    print(name, "truncations bit-equal to the recording:", n, "of 6 | so far over the fixtures:",
          sum(_exact.values()), "of", 6 * len(_exact))


# ------------------------------------------------ b. entry against the twin --
def _small(dt, V):
    """V vertices without an edge, an l1 term"""
    z = np.zeros(0, np.int32)
    y = (np.arange(V) % 3 - 0.75).astype(dt)
    return dict(kind="duplex", V=V, E=0, N=0, K=0, dtype=dt, CP_itMax=3, PFDR_itMax=2000,
                positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3,
                difRcd=0.0, Y=y, A=None, Eu=z, Ev=z, La_d1=np.zeros(0, dt),
                La_l1=np.full(V, 0.02, dt))


def _24x20(dt, **over):
    return P.problem("duplex", "diag", dt, nx=24, ny=20, **over)


PATHS = {
    "direct12": lambda dt: RC.problem("direct12", dt),
    "direct160": lambda dt: RC.problem("direct160", dt),
    "AtA": lambda dt: RC.problem("AtA", dt),
    "pos_diag": lambda dt: _24x20(dt, La_l1=None, positivity=1),  # positivity without La_l1
    "l1pos_diag": lambda dt: RC.problem("l1pos_diag", dt),
    "tiny_tol": lambda dt: _24x20(dt, CP_difTol=1e-9, CP_itMax=4),
    "zero_tol": lambda dt: _24x20(dt, CP_difTol=0.0, CP_itMax=3),
    "nothing": lambda dt: RC.problem("nothing", dt),
    "E0_V5": lambda dt: _small(dt, 5),
    "E0_V1": lambda dt: _small(dt, 1),
}
PATH_IDS = [(k, dt) for k in PATHS for dt in (F32, F64) if not (k == "tiny_tol" and dt is F64)]
_ids = ["%s_%s" % (k, "f32" if dt is F32 else "f64") for k, dt in PATH_IDS]
_cache = {}


def path_case(kind, dt):
    """-> (problem, twin's rX0, twin's records, the entry's full run), once per case"""
    key = (kind, dt)
    if key not in _cache:
        p = PATHS[kind](dt)
        t = DT.gpu_twin(p)
        rX0, recs = t.run(p["CP_itMax"])
        t.b.close()
        _cache[key] = (p, rX0, recs, entry(p))
    return _cache[key]


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_entry_is_the_twin(gpu_lib, kind, dt):
    """Both sides run the same library, so any difference is a wiring
    difference.  The twin goes through the host-memory entries; the driver
    through device memory and a session."""
    p, rX0, recs, full = path_case(kind, dt)
    K = p["CP_itMax"]
    print(kind, np.dtype(dt).name, "twin: rV", [r["rV"] for r in recs], "preAt",
          [r["preAt"] for r in recs], "activated", [r["activated"] for r in recs], "PFDR it",
          [r["pfdr_it"] for r in recs])
    assert all(len(r["segments"]) == 1 and r["segments"][0].size == 2 * p["V"] for r in recs)
    for k in range(1, K + 1):
        Cv, rX, it, Obj, Dif, Time = full if k == K else entry(p, CP_itMax=k)
        assert it == min(k, len(recs)), (k, it, len(recs))
        assert same_bytes(Cv, recs[it - 1]["Cv"]), (k, it)
        assert same_bytes(rX, recs[it - 1]["rX"]), (k, it)
    # CP_itMax = 0: initialize() alone
    Cv, rX, it, Obj, Dif, Time = entry(p, CP_itMax=0)
    assert it == 0 and not Cv.any() and same_bytes(rX, rX0)
    taken = [r["preAt"] for r in recs if r["preAt"] is not None]
    if kind == "direct12":
        assert True in taken and False in taken, taken
    if kind in ("AtA", "pos_diag", "l1pos_diag"):
        assert taken and all(taken), taken
    if kind in ("pos_diag", "l1pos_diag"):
        assert np.all(full[1] >= 0) and recs[-1]["rV"] > 1
    if kind == "zero_tol":
        assert full[2] == 3 and len(recs) == 3
    if kind == "tiny_tol":
        assert DT.real_eps(dt, p["CP_difTol"]) == dt(1e-9)
    if kind in ("nothing", "E0_V5", "E0_V1"):
        Cv, rX, it, Obj, Dif, Time = full
        assert rX.size == 1 and it == 1 and not Cv.any()
        assert Dif[0] == 0 and Obj[1] == Obj[0]
        assert same_bytes(rX, rX0)
        assert recs[0]["activated"] == 0


# ---------------------------- c. against the reference's own recorded run --
@pytest.mark.parametrize("name", [n for n in RC.NAMES if n.startswith(("l1pos_diag", "nothing"))])
def test_recorded_run_exact(gpu_lib, name):
    """N = 0: Cv, rX and CP_it of the reference's run, exactly"""
    p = RC.by_name(name)
    g = RC.load(name)
    Cv, rX, it, Obj, Dif, Time = entry(p)
    assert it == g["CP_it"]
    assert np.array_equal(Cv, g["Cv"])
    assert rX.dtype == g["rX"].dtype and np.array_equal(rX, g["rX"])


@pytest.mark.parametrize("kind", ["direct12", "direct160", "AtA"])
@pytest.mark.parametrize("d", ["f32", "f64"])
def test_recorded_run_functional(gpu_lib, kind, d):
    """N != 0: L comes from a power iteration that matches the reference's
    (time-seeded) one to 2e-2 only, so rX is not owed bit for bit: Cv and CP_it
    equal, and |F(GPU) - F(ref f64)| <= max(1e-5, 4 gap_ref) |F(ref f64)| in f64
    on the f64 problem, gap_ref the relative difference between the reference's
    own f32 and f64 recorded runs (the rule of test_cut_pursuit_gpu.py)."""
    p = RC.problem(kind, RC.DTYPES[d])
    p64 = RC.problem(kind, F64)
    g32, g64 = RC.load(kind + "_f32"), RC.load(kind + "_f64")
    Cv, rX, it, Obj, Dif, Time = entry(p)
    g = RC.load("%s_%s" % (kind, d))
    F64r, F32r, Fg = (functional(p64, np.asarray(x, F64)[c]) for x, c in (
        (g64["rX"], g64["Cv"]), (g32["rX"], g32["Cv"]), (rX, Cv)))
    gap_ref = abs(F32r - F64r) / abs(F64r)
    gap = (Fg - F64r) / abs(F64r)
    print("%s_%s F ref f64 %.9g f32 %.9g GPU %.9g gap_ref %.3e gap %.3e; CP_it GPU %d ref %d; "
          "rV GPU %d ref %d; vertices in another component %d" % (
              kind, d, F64r, F32r, Fg, gap_ref, gap, it, g["CP_it"], rX.size, g["rX"].size,
              relabel_differences(Cv, g["Cv"])))
    assert abs(Fg - F64r) <= max(REL, 4 * gap_ref) * abs(F64r)
    assert it == g["CP_it"] and rX.size == g["rX"].size
    assert relabel_differences(Cv, g["Cv"]) == 0


# ------------------------------------------------ d. differentiable case --
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_differentiable_case_is_the_l1_entry(gpu_lib, dt):
    p = P.problem("duplex", "diag", dt, nx=48, ny=40, La_l1=None)
    assert p["La_l1"] is None and not p["positivity"]
    a, b = entry(p), l1_entry(p)
    assert a[2] == b[2] >= 1 and a[1].size > 1
    for x, y in zip(a[:5], b[:5]):  # Cv, rX, CP_it, Obj, Dif
        assert same_bytes(np.asarray(x), np.asarray(y))
    s = pfdr.Lib().cp_quadratic_d1_l1_duplex_stats()
    assert s["n_cuts"] == a[2]


# ------------------------------------- e. Obj and Dif against f64, bounded --
@pytest.mark.parametrize("kind,dt", [("direct12", F32), ("l1pos_diag", F64)],
                         ids=["direct12_f32", "l1pos_diag_f64"])
def test_obj_and_dif_at_every_iteration(gpu_lib, kind, dt):
    p, rX0, recs, full = path_case(kind, dt)
    check_obj_dif("%s_%s" % (kind, np.dtype(dt).name), p, rX0, recs, full)


# --------------- f. optional outputs, argument errors and repeatability, raw --
def raw(p, Obj=True, Dif=True, Time=True, CP_it=True, **over):
    """pfdr_cp_quadratic_d1_l1_duplex_* through ctypes -> (status, Cv, rX, CP_it or None)"""
    q = dict(p)
    q.update(over)
    dt = np.dtype(q["dtype"])
    ct = C.c_float if dt == F32 else C.c_double
    fn = getattr(pfdr.load(),
                 "pfdr_cp_quadratic_d1_l1_duplex_" + ("f32" if dt == F32 else "f64"))
    V, K = q["V"], max(q["CP_itMax"], 0)
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    Y, A, La, L1 = (arr(q[k], dt) for k in ("Y", "A", "La_d1", "La_l1"))
    Eu, Ev = arr(q["Eu"], np.int32), arr(q["Ev"], np.int32)
    Cv, rX = np.full(max(V, 1), -1, np.int32), np.zeros(max(V, 1), dt)
    o, d, t = np.zeros(K + 1, dt), np.zeros(max(K, 1), dt), np.zeros(K + 1)
    rV, it = C.c_int(0), C.c_int(-1)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    st = fn(C.c_int(V), C.c_int(q["E"]), C.c_int(q["N"]), C.byref(rV), ptr(Cv), ptr(rX), ptr(Y),
            ptr(A), ptr(Eu), ptr(Ev), ptr(La), ptr(L1), C.c_int(q["positivity"]),
            ct(q["CP_difTol"]), C.c_int(q["CP_itMax"]), C.byref(it) if CP_it else None,
            ct(q["rho"]), ct(q["condMin"]), ct(q["difRcd"]), ct(q["PFDR_difTol"]),
            C.c_int(q["PFDR_itMax"]), ptr(t) if Time else None, ptr(o) if Obj else None,
            ptr(d) if Dif else None, C.c_int(0))
    return st, Cv[:max(V, 0)], rX[:rV.value].copy(), it.value if CP_it else None


def test_optional_outputs_and_repeatability(gpu_lib):
    p = _24x20(F32, positivity=1)
    st, Cv, rX, it = raw(p)
    assert st == 0 and 1 <= it <= p["CP_itMax"] and rX.size > 1
    st, Cv2, rX2, it2 = raw(p)  # two runs, the same bytes
    assert st == 0 and it2 == it and same_bytes(Cv2, Cv) and same_bytes(rX2, rX)
    for off in ({"Obj": False}, {"Dif": False}, {"Time": False}, {"CP_it": False},
                {"Obj": False, "Dif": False, "Time": False, "CP_it": False}):
        st, Cv2, rX2, it2 = raw(p, **off)
        assert st == 0, off
        assert same_bytes(Cv2, Cv) and same_bytes(rX2, rX), off
        if off.get("CP_it", True):
            assert it2 == it
    # Dif == NULL and CP_difTol == 0: nothing is tracked, the run goes to CP_itMax
    st, Cv0, rX0, it0 = raw(p, Dif=False, CP_difTol=0.0, CP_itMax=3)
    assert st == 0 and it0 == 3
    st, Cv1, rX1, it1 = raw(p, CP_difTol=0.0, CP_itMax=3)
    assert st == 0 and it1 == 3 and same_bytes(Cv0, Cv1) and same_bytes(rX0, rX1)


def test_argument_errors(gpu_lib):
    p = _24x20(F32)
    pA = RC.problem("AtA", F32)
    bad = [
        ("V <= 0", p, dict(V=0)),
        ("V <= 0", p, dict(V=-3)),
        ("CP_itMax < 0", p, dict(CP_itMax=-1)),
        ("N != 0 without A", p, dict(N=7, A=None)),
        ("N != 0 without A", pA, dict(A=None)),
        ("N < 0, -N != V", pA, dict(N=-(pA["V"] - 1))),
        ("E > 0 without Eu", p, dict(Eu=None)),
    ]
    for what, q, over in bad:
        st, Cv, rX, it = raw(q, **over)
        msg = pfdr.load().pfdr_last_error().decode()
        assert st == 1, (what, st)  # PFDR_ERR_ARG
        assert msg.startswith("pfdr_cp_quadratic_d1_l1_duplex_f32: "), (what, msg)
    # the library is still usable
    st, Cv, rX, it = raw(p)
    assert st == 0 and it >= 1 and rX.size == Cv.max() + 1


def test_verbose_prints_the_l1_entrys_lines(gpu_lib, capfd):
    p = RC.problem("l1pos_diag", F32)
    a = entry(p)
    args, kw = _args(p, None)
    b = pfdr.Lib().cp_quadratic_d1_l1_duplex(*args, verbose=1000, **kw)
    out = capfd.readouterr().out
    assert a[2] == b[2] and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    assert out.count("Cut pursuit iteration") == a[2] + 1, out
    assert "1 connected component(s), 0 reduced edge(s)" in out
    assert "DIFFERENTIABLE" not in out.upper()


# ------------------------------------------------------------ g. the stats --
@pytest.mark.parametrize("kind", ["direct12", "l1pos_diag", "nothing"])
def test_stats(gpu_lib, kind):
    p = RC.problem(kind, F32)
    lib = pfdr.Lib()
    Cv, rX, it, Obj, Dif, Time = entry(p)
    s = lib.cp_quadratic_d1_l1_duplex_stats()
    phases = [s[k] for k in ("gradient", "cuts", "graph", "pfdr", "sums")]
    assert all(x >= 0 for x in phases) and s["total"] > 0
    assert sum(phases) <= s["total"]
    assert Time[it] <= s["total"]
    assert s["n_cuts"] == it  # one two-layer cut per iteration run
    assert s["rounds"] >= 0 and s["relabels"] >= it
    if kind == "nothing":
        assert s["pfdr_it"] == 0 and s["pfdr"] == 0
    else:
        assert s["pfdr_it"] > 0 and s["pfdr"] > 0 and s["rounds"] > 0
    # the l1 entry leaves this thread's duplex record alone
    l1_entry(p, CP_itMax=1)
    assert lib.cp_quadratic_d1_l1_duplex_stats() == s
    # either output may be NULL
    raw_fn = pfdr.load().pfdr_cp_quadratic_d1_l1_duplex_stats
    cnt = np.zeros(4, np.int64)
    assert raw_fn(None, None) == 0
    assert raw_fn(None, C.c_void_p(cnt.ctypes.data)) == 0
    assert cnt.tolist() == [s["n_cuts"], s["rounds"], s["relabels"], s["pfdr_it"]]


# ------------------------------------------------------ h. the front ends --
PAR = (1e-4, 4, 1.5, 1e-3, 0.0, 1e-5, 2000)  # CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax


def _same_result(got, want):
    Cv, rX, it, Time, Obj, Dif = got
    wCv, wrX, wit, wObj, wDif, wTime = want
    assert it == wit and same_bytes(Cv, wCv) and same_bytes(rX, wrX)
    assert Time is not None and Time.size == PAR[1] + 1
    assert same_bytes(Dif, wDif)
    return Obj, wObj


def test_mex_quadratic(gpu_lib):
    p = RC.problem("direct12", F32)
    A = np.asarray(p["A"]).reshape(p["V"], p["N"]).T  # N-by-V
    got = pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex(
        p["Y"], A, p["Eu"], p["Ev"], p["La_d1"], p["La_l1"], 0, *PAR, time=True, obj=True,
        dif=True)
    Obj, wObj = _same_result(got, entry(p, CP_itMax=PAR[1]))
    assert same_bytes(Obj, wObj)
    Cv, rX, it, Time, Obj, Dif = pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex(
        p["Y"], A, p["Eu"], p["Ev"], p["La_d1"], p["La_l1"], 0, *PAR)
    assert Time is None and Obj is None and Dif is None and same_bytes(rX, got[1])


def test_mex_l22(gpu_lib):
    p = P.problem("duplex", "identity", F32, nx=24, ny=18, positivity=1)
    V = p["V"]
    w = (0.5 + np.arange(V) % 4 / 4.0).astype(F32)
    y = np.asarray(p["Y"], F32)
    got = pfdr.CP_PFDR_graph_l22_d1_l1_duplex(y, w, p["Eu"], p["Ev"], p["La_d1"], p["La_l1"], 1,
                                              *PAR, time=True, obj=True, dif=True)
    q = dict(p, Y=(w * y).astype(F32), A=w)
    want = entry(q, CP_itMax=PAR[1])
    Obj, wObj = _same_result(got, want)
    it = got[2]
    y2 = float(np.sum(w.astype(F64) * y * y)) / 2.0
    expect = wObj.copy()
    expect[: it + 1] += y2
    assert same_bytes(Obj, expect)
    # a scalar La_l2: no weights, the identity; a scalar La_l1: no l1 term
    got1 = pfdr.CP_PFDR_graph_l22_d1_l1_duplex(y, 1.0, p["Eu"], p["Ev"], p["La_d1"], 0.0, 1, *PAR)
    want1 = entry(dict(p, La_l1=None), CP_itMax=PAR[1])
    assert got1[2] == want1[2] and same_bytes(got1[0], want1[0]) and same_bytes(got1[1], want1[1])


def test_binding_conventions(gpu_lib):
    """CP_quadratic_l1_duplex: CP_quadratic_l1's conventions through _binding_inputs"""
    p = _24x20(F32, positivity=1)
    V = p["V"]
    y = (np.asarray(p["Y"]) / np.asarray(p["A"])).astype(F32)
    a = np.sqrt(np.asarray(p["A"], F64)).astype(F32)
    kw = dict(positivity=1, PFDR_rho=1.5, CP_difTol=1e-4, PFDR_difTol=1e-5, CP_itMax=4,
              PFDR_itMax=2000)
    # a vector A: the diagonal, obs and A premultiplied (obs * A, A * A)
    Cv, rX = pfdr.CP_quadratic_l1_duplex(y, p["Eu"].astype(np.uint32), p["Ev"].astype(np.uint32),
                                         0.3, a, 0.02, **kw)
    q = dict(p, Y=(y * a).astype(F32), A=(a * a).astype(F32), CP_itMax=4)
    want = entry(q)
    assert Cv.dtype == np.uint32 and np.array_equal(Cv, want[0]) and same_bytes(rX, want[1])
    # a scalar A: the identity, its value discarded
    Cv, rX = pfdr.CP_quadratic_l1_duplex(y, p["Eu"], p["Ev"], p["La_d1"], 3.0, p["La_l1"], **kw)
    want = entry(dict(p, Y=y, A=None, CP_itMax=4))
    assert np.array_equal(Cv, want[0]) and same_bytes(rX, want[1])
