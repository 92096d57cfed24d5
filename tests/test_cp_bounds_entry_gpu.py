"""The bounds driver's one-call cut pursuit (pfdr_cp_quadratic_d1_bounds,
the bounds flavour of csrc/pfdr_cutpursuit.hip) pinned on every path of its loop.

a. N = 0: Cv, rX and CP_it equal the reference's recorded iterations
   (tests/golden/cp_bounds_*.npz) bit for bit, for every truncation
   CP_itMax = 1..6 of all ten fixtures.
b. Entry against the step-composed twin (tests/cp_bounds_twin.py over the
   library's own per-step API): Cv, rX, CP_it and Dif byte-identical for every
   truncation CP_itMax = 0..K, on the nine recorded-run cases in both types and
   on CP_difTol below machine eps, CP_difTol == 0, min == max, E == 0 and
   V == 1.
c. Entry against the reference's own recorded runs (tests/golden/cp_bounds_run/):
   exact for N = 0; equal Cv and CP_it and a bound on the functional otherwise.
d. Obj[k] and Dif[k] at every iteration against f64, within a derived rounding
   bound.
e. Every component value lies in the box; the components the reference left
   at a bound sit exactly on it.
f. Optional outputs (NULL), argument errors and repeatability through ctypes.
g. The stats call.
h. The three MEX-named front-ends.
"""
import ctypes as C

import numpy as np
import pytest

import cp_bounds_run_cases as RC
import cp_bounds_twin as BT
import cp_problems as P
from cp_pfdr_graph_d1_amd import pfdr
from test_cp_graph_oracle import BNAMES, load_case
from test_cut_pursuit_gpu import functional
# The rounding bounds of the l1 entry's test, derived there (obj_bound,
# dif_bound).  They hold here term for term: this driver forms the same sums in
# the same order -- the one-component value from V-term sums (rY, rAA; for
# N > 0 through the column sums rA), 1/2 sum R^2 with R = Y - sum_rv rA x,
# sum_rv x (1/2 rAA x - rY) or its full-matrix form, sum_re rLa |x_ru - x_rv| --
# without an l1 term (its bound is then 0), and Obj = quad + d1 costs one
# rounding of the partial sums where obj_bound counts two.  The projection of
# the one-component value onto the box is exact (it returns min, max or the
# value), and F is evaluated at the projected value on both sides.
from test_cut_pursuit_paths_gpu import check_obj_dif, same_bytes

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
REL = 1e-5  # the project's parity bar
# the iteration fixtures' recorder parameters (oracle.CPStepRefBounds.step defaults)
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=1000)
inf = float("inf")


def entry(p, CP_itMax=None, **over):
    q = dict(p)
    q.update(over)
    return pfdr.Lib().cp_quadratic_d1_bounds(
        q["V"], q["N"], q["Y"], q["A"], q["Eu"], q["Ev"], q["La_d1"], lo=q["lo"], hi=q["hi"],
        CP_difTol=q["CP_difTol"], CP_itMax=q["CP_itMax"] if CP_itMax is None else CP_itMax,
        rho=q["rho"], condMin=q["condMin"], difRcd=q["difRcd"], difTol=q["PFDR_difTol"],
        itMax=q["PFDR_itMax"])


def fixture_problem(c):
    """an iteration fixture's inputs as a cp_problems dict"""
    dt = c["Y"].dtype.type
    return dict(kind="bounds", V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=dt, CP_itMax=6,
                PFDR_itMax=STEP["itMax"], positivity=0, CP_difTol=c["CP_difTol"],
                PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
                difRcd=STEP["difRcd"], lo=c["lo"], hi=c["hi"], Y=c["Y"], A=c["A"], Eu=c["Eu"],
                Ev=c["Ev"], La_d1=c["La_d1"], La_l1=None)


def in_box(p, rX):
    real = np.dtype(p["dtype"]).type
    return bool(np.all(rX >= real(p["lo"])) and np.all(rX <= real(p["hi"])))


# ------------------------------------------ a. exact against the reference --
@pytest.mark.parametrize("name", BNAMES)
def test_entry_is_the_reference_run(gpu_lib, name):
    """N = 0: every cut returns the reference's segments, PFDR is bit-exact in
    the graph modes and L is rAA itself, so the entry owes the reference's Cv,
    rX and CP_it exactly.  tests/test_cp_bounds_twin_cpu.py checks that the
    recorded warm-restart chain is the reference's one-call run, which stops
    early in none of the 60 truncations."""
    c, d = load_case(name)
    p = fixture_problem(c)
    assert int(d["meta_steps"]) == 6
    for k in range(1, 7):
        Cv, rX, it, Obj, Dif, Time = entry(p, CP_itMax=k)
        assert it == k, (k, it, Dif[:it])
        assert np.array_equal(Cv, d["k%d_out_Cv" % (k - 1)]), k
        want = d["k%d_out_rX" % (k - 1)]
        assert rX.dtype == want.dtype and np.array_equal(rX, want), k
        assert in_box(p, rX), k
    # e. the final state: what the reference left at a bound sits exactly on it
    real = rX.dtype.type
    for b in (real(c["lo"]), real(c["hi"])):
        assert np.array_equal(rX == b, want == b)


def test_all_ten_fixtures_are_run():
    assert len(BNAMES) == 10, BNAMES


# ------------------------------------------------ b. entry against the twin --
def _small(dt, V):
    """V vertices without an edge"""
    z = np.zeros(0, np.int32)
    y = (np.arange(V) % 3 - 0.75).astype(dt)
    return dict(kind="bounds", V=V, E=0, N=0, K=0, dtype=dt, CP_itMax=3, PFDR_itMax=2000,
                positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3,
                difRcd=0.0, lo=-0.3, hi=0.8, Y=y, A=None, Eu=z, Ev=z, La_d1=np.zeros(0, dt),
                La_l1=None)


def _diag_24x20(dt, **over):
    return P.problem("bounds", "diag", dt, nx=24, ny=20, **over)


PATHS = {k: (lambda dt, k=k: RC.problem(k, dt)) for k in RC.KINDS}
PATHS.update({
    "tiny_tol": lambda dt: _diag_24x20(dt, CP_difTol=1e-9, CP_itMax=4),
    "zero_tol": lambda dt: _diag_24x20(dt, CP_difTol=0.0, CP_itMax=3),
    "min_eq_max": lambda dt: _diag_24x20(dt, lo=0.25, hi=0.25, CP_itMax=3),
    "E0_V5": lambda dt: _small(dt, 5),
    "E0_V1": lambda dt: _small(dt, 1),
})
PATH_IDS = [(k, dt) for k in PATHS for dt in (F32, F64) if not (k == "tiny_tol" and dt is F64)]
_ids = ["%s_%s" % (k, "f32" if dt is F32 else "f64") for k, dt in PATH_IDS]
_cache = {}


def path_case(kind, dt):
    """-> (problem, twin's rX0, twin's records, the entry's full run), once per case"""
    key = (kind, dt)
    if key not in _cache:
        p = PATHS[kind](dt)
        t = BT.gpu_twin(p)
        rX0, recs = t.run(p["CP_itMax"])
        t.b.close()
        _cache[key] = (p, rX0, recs, entry(p))
    return _cache[key]


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_entry_is_the_twin(gpu_lib, kind, dt):
    """Both sides run the same library, so any difference is a wiring
    difference.  The twin goes through the host-memory entries; the driver
    through device memory and a session: the same solver class either way."""
    p, rX0, recs, full = path_case(kind, dt)
    K = p["CP_itMax"]
    print(kind, np.dtype(dt).name, "twin: rV", [r["rV"] for r in recs], "preAt",
          [r["preAt"] for r in recs], "activated", [r["activated"] for r in recs], "PFDR it",
          [r["pfdr_it"] for r in recs])
    difs = np.array([r["dif"] for r in recs], dt)
    for k in range(1, K + 1):
        Cv, rX, it, Obj, Dif, Time = full if k == K else entry(p, CP_itMax=k)
        assert it == min(k, len(recs)), (k, it, len(recs))
        assert same_bytes(Cv, recs[it - 1]["Cv"]), (k, it)
        assert same_bytes(rX, recs[it - 1]["rX"]), (k, it)
        assert same_bytes(Dif[:it], difs[:it]), (k, it, Dif[:it], difs[:it])
        assert in_box(p, rX), (k, it)
    # CP_itMax = 0: initialize() alone, the one-component value projected on the box
    Cv, rX, it, Obj, Dif, Time = entry(p, CP_itMax=0)
    assert it == 0 and not Cv.any() and same_bytes(rX, rX0) and in_box(p, rX)
    # the preAt rule (:648) from the twin's own records, PFDR_it from the call before
    taken, pit = [], p["PFDR_itMax"]
    for r in recs:
        if r["preAt"] is None:
            continue
        N = p["N"]
        assert r["preAt"] == (N <= 0 or r["rV"] < (2 * N * pit) // (N + pit)), (r["rV"], pit)
        taken.append(r["preAt"])
        pit = r["pfdr_it"]
    real = np.dtype(dt).type
    if kind == "direct12":
        assert True in taken and False in taken, taken
    if kind in ("AtA", "clamp_lo", "clamp_hi", "free_diag", "early"):
        assert taken and all(taken), taken
    if kind == "clamp_lo":   # the start is clamped to lo
        assert rX0[0] == real(p["lo"])
    if kind == "clamp_hi":
        assert rX0[0] == real(p["hi"])
    if kind == "free_diag":  # one cut per iteration
        assert all(len(r["segments"]) == 1 for r in recs)
    elif kind not in ("E0_V5", "E0_V1"):
        assert all(len(r["segments"]) == 2 for r in recs)
    if kind == "early":      # stopped on the iterate evolution
        assert full[2] < K and full[4][full[2] - 1] < real(p["CP_difTol"]) ** 2
    if kind == "zero_tol":
        assert full[2] == 3 and len(recs) == 3
    if kind == "tiny_tol":
        assert BT.real_eps(dt, p["CP_difTol"]) == dt(1e-9)
    if kind in ("nothing", "pinned", "min_eq_max", "E0_V5", "E0_V1"):
        Cv, rX, it, Obj, Dif, Time = full
        assert rX.size == 1 and not Cv.any()
        assert Dif[0] == 0 and Obj[1] == Obj[0]
        assert same_bytes(rX, rX0)
        assert recs[0]["activated"] == 0
    if kind in ("pinned", "min_eq_max"):
        assert full[1][0] == real(p["lo"])


# ---------------------------- c. against the reference's own recorded run --
@pytest.mark.parametrize("name", [n for n in RC.NAMES if RC.by_name(n)["N"] == 0])
def test_recorded_run_exact(gpu_lib, name):
    """N = 0: Cv, rX and CP_it of the reference's run, exactly"""
    p = RC.by_name(name)
    g = RC.load(name)
    kind, d = name.rsplit("_", 1)
    Cv, rX, it, Obj, Dif, Time = path_case(kind, RC.DTYPES[d])[3]
    assert it == g["CP_it"]
    assert np.array_equal(Cv, g["Cv"])
    assert rX.dtype == g["rX"].dtype and np.array_equal(rX, g["rX"])
    assert RC.at_bounds(p, rX) == RC.EXPECT[kind][2:]


@pytest.mark.parametrize("kind", ["direct12", "direct160", "AtA"])
@pytest.mark.parametrize("d", ["f32", "f64"])
def test_recorded_run_functional(gpu_lib, kind, d):
    """N != 0: L comes from a power iteration that matches the reference's
    (time-seeded) one to 2e-2 only, so rX is not owed bit for bit.  CP_it and Cv
    are equal, and |F(GPU) - F(ref f64)| <= max(1e-5, 4 gap_ref) |F(ref f64)| in
    f64 on the f64 problem, gap_ref the relative difference between the
    reference's own f32 and f64 recorded runs.  e: the components the reference
    left at a bound are the entry's, exactly on it."""
    p = RC.problem(kind, RC.DTYPES[d])
    p64 = RC.problem(kind, F64)
    g32, g64 = RC.load(kind + "_f32"), RC.load(kind + "_f64")
    Cv, rX, it, Obj, Dif, Time = path_case(kind, RC.DTYPES[d])[3]
    g = RC.load("%s_%s" % (kind, d))
    F64r, F32r, Fg = (functional(p64, np.asarray(x, F64)[c]) for x, c in (
        (g64["rX"], g64["Cv"]), (g32["rX"], g32["Cv"]), (rX, Cv)))
    gap_ref = abs(F32r - F64r) / abs(F64r)
    gap = (Fg - F64r) / abs(F64r)
    print("%s_%s F ref f64 %.9g f32 %.9g GPU %.9g gap_ref %.3e gap %.3e; CP_it GPU %d ref %d; "
          "rV GPU %d ref %d; vertices in another component %d; at lo / hi GPU %s ref %s" % (
              kind, d, F64r, F32r, Fg, gap_ref, gap, it, g["CP_it"], rX.size, g["rX"].size,
              int(np.count_nonzero(Cv != g["Cv"])), RC.at_bounds(p, rX),
              RC.at_bounds(p, g["rX"])))
    assert it == g["CP_it"]
    assert np.array_equal(Cv, g["Cv"])
    assert abs(Fg - F64r) <= max(REL, 4 * gap_ref) * abs(F64r)
    assert in_box(p, rX)
    real = rX.dtype.type
    for b in (real(p["lo"]), real(p["hi"])):
        assert np.array_equal(rX == b, g["rX"] == b), b


# ------------------------------------- d. Obj and Dif against f64, bounded --
@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_obj_and_dif_at_every_iteration(gpu_lib, kind, dt):
    """Obj[k] against the functional of the k-th iterate and Dif[k-1] against
    sum (x_k - x_{k-1})^2 / max(sum x_k^2, eps), both in f64, x_k the twin's k-th
    iterate (byte-equal to the entry's, test_entry_is_the_twin), within
    gamma_n = n u / (1 - n u) over every sum the driver forms plus the
    yardstick's own bound (see the import above).  N > 0, N == 0 and N < 0 each
    occur."""
    p, rX0, recs, full = path_case(kind, dt)
    check_obj_dif("%s_%s" % (kind, np.dtype(dt).name), p, rX0, recs, full)


@pytest.mark.parametrize("name", ["cp_bounds_box_f32", "cp_bounds_knn_diag_f64"])
def test_obj_and_dif_on_fixtures(gpu_lib, name):
    c, d = load_case(name)
    p = fixture_problem(c)
    t = BT.gpu_twin(p)
    rX0, recs = t.run(p["CP_itMax"])
    t.b.close()
    check_obj_dif(name, p, rX0, recs, entry(p))


# --------------- f. optional outputs, argument errors and repeatability, raw --
def raw(p, Obj=True, Dif=True, Time=True, CP_it=True, **over):
    """pfdr_cp_quadratic_d1_bounds_* through ctypes -> (status, Cv, rX, CP_it or
    None); Cv starts at -1 and rX at 7 everywhere: untouched outputs show"""
    q = dict(p)
    q.update(over)
    dt = np.dtype(q["dtype"])
    ct = C.c_float if dt == F32 else C.c_double
    fn = getattr(pfdr.load(), "pfdr_cp_quadratic_d1_bounds_" + ("f32" if dt == F32 else "f64"))
    V, K = q["V"], max(q["CP_itMax"], 0)
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    Y, A, La = (arr(q[k], dt) for k in ("Y", "A", "La_d1"))
    Eu, Ev = arr(q["Eu"], np.int32), arr(q["Ev"], np.int32)
    Cv, rX = np.full(max(V, 1), -1, np.int32), np.full(max(V, 1), 7, dt)
    o, d, t = np.zeros(K + 1, dt), np.zeros(max(K, 1), dt), np.zeros(K + 1)
    rV, it = C.c_int(-5), C.c_int(-1)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    st = fn(C.c_int(V), C.c_int(q["E"]), C.c_int(q["N"]), C.byref(rV), ptr(Cv), ptr(rX), ptr(Y),
            ptr(A), ptr(Eu), ptr(Ev), ptr(La), ct(q["lo"]), ct(q["hi"]), ct(q["CP_difTol"]),
            C.c_int(q["CP_itMax"]), C.byref(it) if CP_it else None, ct(q["rho"]),
            ct(q["condMin"]), ct(q["difRcd"]), ct(q["PFDR_difTol"]), C.c_int(q["PFDR_itMax"]),
            ptr(t) if Time else None, ptr(o) if Obj else None, ptr(d) if Dif else None,
            C.c_int(0))
    if st != 0:  # nothing may have been written
        assert rV.value == -5 and it.value == -1
        assert np.all(Cv == -1) and np.all(rX == 7)
        assert not o.any() and not d.any() and not t.any()
        return st, Cv, rX, None
    return st, Cv[:max(V, 0)], rX[:rV.value].copy(), it.value if CP_it else None


def test_optional_outputs_and_repeatability(gpu_lib):
    p = P.problem("bounds", "diag", F32, nx=24, ny=20)
    st, Cv, rX, it = raw(p)
    assert st == 0 and 1 <= it <= p["CP_itMax"]
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
    # a dense problem too
    q = RC.problem("direct12", F32)
    a, b = raw(q, CP_itMax=3), raw(q, CP_itMax=3, Obj=False, Dif=False, Time=False)
    assert a[0] == 0 and b[0] == 0 and same_bytes(a[1], b[1]) and same_bytes(a[2], b[2])


def test_verbose_changes_nothing(gpu_lib, capfd):
    p = RC.problem("clamp_lo", F32)
    a = entry(p)
    q = dict(p)
    b = pfdr.Lib().cp_quadratic_d1_bounds(
        q["V"], q["N"], q["Y"], q["A"], q["Eu"], q["Ev"], q["La_d1"], lo=q["lo"], hi=q["hi"],
        CP_difTol=q["CP_difTol"], CP_itMax=q["CP_itMax"], rho=q["rho"], condMin=q["condMin"],
        difRcd=q["difRcd"], difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"], verbose=1000)
    out = capfd.readouterr().out
    assert a[2] == b[2] and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    # the l1 entry's lines, one block per iteration and the closing one
    assert out.count("Cut pursuit iteration") == a[2] + 1, out
    assert "Cut pursuit iteration 0 (max. %d)" % p["CP_itMax"] in out
    assert "1 connected component(s), 0 reduced edge(s)" in out
    assert "relative iterate evolution" in out


def test_argument_errors(gpu_lib):
    p = P.problem("bounds", "diag", F32, nx=24, ny=20)
    pA = RC.problem("AtA", F32)
    bad = [
        ("V <= 0", p, dict(V=0)),
        ("V <= 0", p, dict(V=-3)),
        ("E < 0", p, dict(E=-1)),
        ("CP_itMax < 0", p, dict(CP_itMax=-1)),
        ("N != 0 without A", p, dict(N=7, A=None)),
        ("N != 0 without A", pA, dict(A=None)),
        ("N < 0, -N != V", pA, dict(N=-(pA["V"] - 1))),
        ("E > 0 without Eu", p, dict(Eu=None)),
        ("E > 0 without Ev", p, dict(Ev=None)),
        ("E > 0 without La_d1", p, dict(La_d1=None)),
        ("no Y", p, dict(Y=None)),
        ("min > max", p, dict(lo=0.5, hi=0.25)),
        ("min > max", p, dict(lo=inf, hi=-inf)),
        ("NaN bound", p, dict(lo=float("nan"))),
        ("NaN bound", p, dict(hi=float("nan"))),
    ]
    for what, q, over in bad:
        st, Cv, rX, it = raw(q, **over)
        msg = pfdr.load().pfdr_last_error().decode()
        assert st == 1, (what, st)  # PFDR_ERR_ARG
        assert msg.startswith("pfdr_cp_quadratic_d1_bounds_f32: "), (what, msg)
    # missing output pointers
    fn = pfdr.load().pfdr_cp_quadratic_d1_bounds_f32
    Y = np.ascontiguousarray(p["Y"], F32)
    Cv, rX, rV = np.zeros(p["V"], np.int32), np.zeros(p["V"], F32), C.c_int(0)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for outs in ((None, vp(Cv), vp(rX)), (C.byref(rV), None, vp(rX)), (C.byref(rV), vp(Cv), None)):
        st = fn(C.c_int(p["V"]), C.c_int(0), C.c_int(0), outs[0], outs[1], outs[2], vp(Y), None,
                None, None, None, C.c_float(-1), C.c_float(1), C.c_float(1e-3), C.c_int(2), None,
                C.c_float(1.5), C.c_float(1e-3), C.c_float(0), C.c_float(1e-4), C.c_int(100),
                None, None, None, C.c_int(0))
        assert st == 1
    # the library is still usable; min == max is valid
    st, Cv, rX, it = raw(p)
    assert st == 0 and it >= 1 and rX.size == Cv.max() + 1
    st, Cv, rX, it = raw(p, lo=0.25, hi=0.25)
    assert st == 0 and rX.size == 1 and rX[0] == F32(0.25)


# ------------------------------------------------------------ g. the stats --
@pytest.mark.parametrize("kind", ["direct12", "free_diag", "nothing"])
def test_stats(gpu_lib, kind):
    p = RC.problem(kind, F32)
    lib = pfdr.Lib()
    Cv, rX, it, Obj, Dif, Time = entry(p)
    s = lib.cp_quadratic_d1_bounds_stats()
    phases = [s[k] for k in ("gradient", "cuts", "graph", "pfdr", "sums")]
    assert all(x >= 0 for x in phases) and s["total"] > 0
    assert sum(phases) <= s["total"]
    assert Time[it] <= s["total"]
    # every iteration reaches the cut: one cut without a bound, two with
    assert s["n_cuts"] == it * (1 if kind == "free_diag" else 2)
    assert s["rounds"] >= 0 and s["relabels"] >= 0
    if kind == "nothing":
        assert s["pfdr_it"] == 0 and s["pfdr"] == 0
    else:
        assert s["pfdr_it"] > 0 and s["pfdr"] > 0 and s["rounds"] > 0
    # either output may be NULL
    raw_fn = pfdr.load().pfdr_cp_quadratic_d1_bounds_stats
    cnt = np.zeros(4, np.int64)
    assert raw_fn(None, None) == 0
    assert raw_fn(None, C.c_void_p(cnt.ctypes.data)) == 0
    assert cnt.tolist() == [s["n_cuts"], s["rounds"], s["relabels"], s["pfdr_it"]]


# ------------------------------------------------- h. the MEX-named front-ends --
PAR = (1e-4, 4, 1.5, 1e-3, 0.0, 1e-5, 2000)  # CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax


def _same_result(got, want, p):
    Cv, rX, it, Time, Obj, Dif = got
    wCv, wrX, wit, wObj, wDif, wTime = want
    assert it == wit and same_bytes(Cv, wCv) and same_bytes(rX, wrX)
    assert Time is not None and Time.size == PAR[1] + 1
    assert same_bytes(Dif, wDif)
    return Obj, wObj


def test_mex_quadratic(gpu_lib):
    p = RC.problem("direct12", F32)
    A = np.asarray(p["A"]).reshape(p["V"], p["N"]).T  # N-by-V
    got = pfdr.CP_PFDR_graph_quadratic_d1_bounds(p["Y"], A, p["Eu"], p["Ev"], p["La_d1"],
                                                 (p["lo"], p["hi"]), *PAR, time=True, obj=True,
                                                 dif=True)
    Obj, wObj = _same_result(got, entry(p, CP_itMax=PAR[1]), p)
    assert same_bytes(Obj, wObj)
    Cv, rX, it, Time, Obj, Dif = pfdr.CP_PFDR_graph_quadratic_d1_bounds(
        p["Y"], A, p["Eu"], p["Ev"], p["La_d1"], (p["lo"], p["hi"]), *PAR)
    assert Time is None and Obj is None and Dif is None and same_bytes(rX, got[1])


def test_mex_AtA(gpu_lib):
    p = RC.problem("AtA", F64)
    V = p["V"]
    AtA = np.asarray(p["A"]).reshape(V, V).T
    got = pfdr.CP_PFDR_graph_quadratic_d1_bounds_AtA(p["Y"], AtA, p["Eu"], p["Ev"], p["La_d1"],
                                                     (p["lo"], p["hi"]), *PAR, time=True,
                                                     obj=True, dif=True)
    Obj, wObj = _same_result(got, entry(p, CP_itMax=PAR[1]), p)
    assert same_bytes(Obj, wObj)


def test_mex_l22(gpu_lib):
    p = P.problem("bounds", "identity", F32, nx=24, ny=18)
    V = p["V"]
    w = (0.5 + np.arange(V) % 4 / 4.0).astype(F32)
    y = np.asarray(p["Y"], F32)
    got = pfdr.CP_PFDR_graph_l22_d1_bounds(y, w, p["Eu"], p["Ev"], p["La_d1"],
                                           (p["lo"], p["hi"]), *PAR, time=True, obj=True,
                                           dif=True)
    q = dict(p, Y=(w * y).astype(F32), A=w)
    want = entry(q, CP_itMax=PAR[1])
    Obj, wObj = _same_result(got, want, q)
    it = got[2]
    y2 = float(np.sum(w.astype(F64) * y * y)) / 2.0
    expect = wObj.copy()
    expect[: it + 1] += y2
    assert same_bytes(Obj, expect)
    # a scalar La_l2: no weights, the identity
    got1 = pfdr.CP_PFDR_graph_l22_d1_bounds(y, 1.0, p["Eu"], p["Ev"], p["La_d1"],
                                            (p["lo"], p["hi"]), *PAR)
    want1 = entry(p, CP_itMax=PAR[1])
    assert got1[2] == want1[2] and same_bytes(got1[0], want1[0]) and same_bytes(got1[1], want1[1])
