"""TEST INFRASTRUCTURE -- the bodies of the tests of the one-call quadratic cut
pursuits (pfdr_cp_quadratic_d1_l1, ..._l1_duplex, ..._bounds: the three
flavours of QuadDriver, csrc/pfdr_cutpursuit.hip), once for all flavours.
tests/test_cut_pursuit_paths_gpu.py (l1), tests/test_cp_duplex_entry_gpu.py and
tests/test_cp_bounds_entry_gpu.py list their own cases and call these with
their flavour; what one flavour asserts more stays under ``if flavour == ...``.
Those modules register this one and cp_entry for pytest's assertion rewriting
before they import them, so a failing ``assert`` here reports its values as it
did when the bodies stood in the test modules.

a. N = 0: Cv, rX and CP_it equal the reference's recorded iterations
   (tests/golden/cp_*.npz, cp_duplex_*.npz, cp_bounds_*.npz) bit for bit, for
   every truncation CP_itMax = 1..6.
b. Entry against the step-composed twin (tests/cp_twin.py over the library's
   own per-step API): Cv, rX, CP_it byte-identical for every truncation
   CP_itMax = 0..K (bounds: Dif too), on the direct branch (preAt == 0), the
   premultiplied dense one, A^tA given, positivity without l1, CP_difTol below
   machine eps, CP_difTol == 0, min == max, a problem with nothing to cut,
   E == 0 and V == 1.
c. Against the reference's own recorded runs (tests/golden/cp_run/,
   cp_duplex_run/, cp_bounds_run/): exact for N = 0, a two-sided bound on the
   functional otherwise.
d. Obj[k] and Dif[k] at every iteration against f64, within a derived
   rounding bound (cp_entry.obj_bound / dif_bound).
e. bounds: every component value lies in the box; the components the reference
   left at a bound sit exactly on it.
f. Optional outputs (NULL), argument errors and repeatability through ctypes.
g. The stats calls.
h. The MEX-named front ends.
"""
import ctypes as C

import numpy as np

import cp_bounds_run_cases
import cp_duplex_run_cases
import cp_problems as P
import cp_run_cases
import cp_twin as T
from cp_entry import (F32, F64, REL, _same_result, check_obj_dif, entry, fixture_problem,
                      functional, raw, relabel_differences, same_bytes)
from cp_fixtures import BNAMES, DNAMES, NAMES, TIES, load_case
from cp_pfdr_graph_d1_amd import pfdr

FLAVOURS = ("l1", "duplex", "bounds")
RUN = {"l1": cp_run_cases, "duplex": cp_duplex_run_cases, "bounds": cp_bounds_run_cases}
FIXTURES = {"l1": NAMES, "duplex": DNAMES, "bounds": BNAMES}
inf = float("inf")


def in_box(p, rX):
    real = np.dtype(p["dtype"]).type
    return bool(np.all(rX >= real(p["lo"])) and np.all(rX <= real(p["hi"])))


def twin_run(p):
    """-> (twin's rX0, twin's records) of the whole run"""
    t = T.gpu_twin(p)
    rX0, recs = t.run(p["CP_itMax"])
    t.b.close()
    return rX0, recs


# ------------------------------------------ a. exact against the reference --
_exact = {"l1": {}, "duplex": {}, "bounds": {}}  # per flavour: fixture -> truncations bit-equal


def entry_is_the_reference_run(flavour, name):
    """N = 0: every cut returns the reference's segments, PFDR is
    bit-exact in the graph modes and L is rAA itself, so the entry owes the
    reference's Cv, rX and CP_it exactly.  tests/test_cp_twin_cpu.py,
    test_cp_duplex_twin_cpu.py and test_cp_bounds_twin_cpu.py check that the
    recorded warm-restart chain is the reference's one-call run; the bounds run
    stops early in none of the 60 truncations.  From the iteration of a cut
    listed in TIES on (a duplex fixture), the truncations are compared with
    the twin."""
    c, d = load_case(name)
    p = fixture_problem(flavour, c)
    tol2 = c["Y"].dtype.type(c["CP_difTol"]) ** 2
    steps = int(d["meta_steps"])
    if flavour == "bounds":
        assert steps == 6
    tie = min([k for n, k in TIES if n == name], default=None)
    recs = None
    if tie is not None:
        _, recs = twin_run(p)
        print(name, "cut %d is a tie between minimum cuts: truncations from CP_itMax = %d on "
              "are compared with the twin, not with the recording" % (tie, tie + 1))
    n = 0
    for k in range(1, steps + 1):
        Cv, rX, it, Obj, Dif, Time = entry(flavour, p, CP_itMax=k)
        assert 1 <= it <= k
        assert it == k or Dif[it - 1] < tol2, (k, it, Dif[:it])
        if flavour == "bounds":
            assert it == k, (k, it, Dif[:it])
        if tie is not None and it - 1 >= tie:
            assert same_bytes(Cv, recs[it - 1]["Cv"]) and same_bytes(rX, recs[it - 1]["rX"])
            continue
        assert np.array_equal(Cv, d["k%d_out_Cv" % (it - 1)]), (k, it)
        want = d["k%d_out_rX" % (it - 1)]
        assert rX.dtype == want.dtype and np.array_equal(rX, want), (k, it)
        if flavour == "bounds":
            assert in_box(p, rX), k
        n += 1
    _exact[flavour][name] = n
    print(name, "truncations bit-equal to the recording:", n, "of 6 | so far over the fixtures:",
          sum(_exact[flavour].values()), "of", 6 * len(_exact[flavour]))
    if flavour == "bounds":
        # e. the final state: what the reference left at a bound sits exactly on it
        real = rX.dtype.type
        for b in (real(c["lo"]), real(c["hi"])):
            assert np.array_equal(rX == b, want == b)


# ------------------------------------------------ b. entry against the twin --
def _small(flavour, dt, V):
    """V vertices without an edge (duplex: an l1 term)"""
    z = np.zeros(0, np.int32)
    y = (np.arange(V) % 3 - 0.75).astype(dt)
    p = dict(kind=flavour, V=V, E=0, N=0, K=0, dtype=dt, CP_itMax=3, PFDR_itMax=2000,
             positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3,
             difRcd=0.0, Y=y, A=None, Eu=z, Ev=z, La_d1=np.zeros(0, dt), La_l1=None)
    if flavour == "duplex":
        p["La_l1"] = np.full(V, 0.02, dt)
    if flavour == "bounds":
        p.update(lo=-0.3, hi=0.8)
    return p


def _24x20(flavour, dt, **over):
    return P.problem(flavour, "diag", dt, nx=24, ny=20, **over)


def _paths(flavour, **own):
    """the flavour's recorded-run problems, its ``own`` paths, and the paths every
    flavour has"""
    run = RUN[flavour]
    paths = {k: (lambda dt, k=k: run.problem(k, dt)) for k in run.KINDS}
    paths.update(own)
    paths.update({
        "tiny_tol": lambda dt: _24x20(flavour, dt, CP_difTol=1e-9, CP_itMax=4),
        "zero_tol": lambda dt: _24x20(flavour, dt, CP_difTol=0.0, CP_itMax=3),
        "E0_V5": lambda dt: _small(flavour, dt, 5),
        "E0_V1": lambda dt: _small(flavour, dt, 1),
    })
    return paths


PATHS = {
    "l1": _paths("l1"),
    # positivity without La_l1
    "duplex": _paths("duplex", pos_diag=lambda dt: _24x20("duplex", dt, La_l1=None, positivity=1)),
    "bounds": _paths("bounds",
                     min_eq_max=lambda dt: _24x20("bounds", dt, lo=0.25, hi=0.25, CP_itMax=3)),
}
PATH_IDS = {f: [(k, dt) for k in PATHS[f] for dt in (F32, F64)
                if not (k == "tiny_tol" and dt is F64)] for f in FLAVOURS}
# the kinds whose every PFDR call is premultiplied, and those that never cut
ALL_PREAT = {"l1": ("AtA", "pos_diag"), "duplex": ("AtA", "pos_diag", "l1pos_diag"),
             "bounds": ("AtA", "clamp_lo", "clamp_hi", "free_diag", "early")}
NO_CUT = {"l1": ("nothing", "E0_V5", "E0_V1"), "duplex": ("nothing", "E0_V5", "E0_V1"),
          "bounds": ("nothing", "pinned", "min_eq_max", "E0_V5", "E0_V1")}
# once per (flavour, kind, dt): the problem with the entry's full run, and the
# twin's run; a flavour's module reads its own keys only
_runs, _twins = {}, {}


def path_ids(ids):
    """[(kind, dt), ...] -> the ids kind_f32 / kind_f64 of a parametrised test"""
    return ["%s_%s" % (k, "f32" if dt is F32 else "f64") for k, dt in ids]


def full_run(flavour, kind, dt):
    """-> (problem, the entry's full run), once per case; no twin is run"""
    key = (flavour, kind, dt)
    if key not in _runs:
        p = PATHS[flavour][kind](dt)
        _runs[key] = (p, entry(flavour, p))
    return _runs[key]


def path_case(flavour, kind, dt):
    """-> (problem, twin's rX0, twin's records, the entry's full run), once per case"""
    key = (flavour, kind, dt)
    p, full = full_run(*key)
    if key not in _twins:
        _twins[key] = twin_run(p)
    return (p,) + _twins[key] + (full,)


def entry_is_the_twin(flavour, kind, dt):
    """Both sides run the same library, so any difference is a wiring
    difference.  The twin goes through the host-memory entries; the driver
    through device memory and a session: the same solver class either way."""
    p, rX0, recs, full = path_case(flavour, kind, dt)
    K = p["CP_itMax"]
    real = np.dtype(dt).type
    print(kind, np.dtype(dt).name, "twin: rV", [r["rV"] for r in recs], "preAt",
          [r["preAt"] for r in recs], "activated", [r["activated"] for r in recs], "PFDR it",
          [r["pfdr_it"] for r in recs])
    if flavour == "duplex":
        assert all(len(r["segments"]) == 1 and r["segments"][0].size == 2 * p["V"] for r in recs)
    for k in range(1, K + 1):
        Cv, rX, it, Obj, Dif, Time = full if k == K else entry(flavour, p, CP_itMax=k)
        assert it == min(k, len(recs)), (k, it, len(recs))
        assert same_bytes(Cv, recs[it - 1]["Cv"]), (k, it)
        assert same_bytes(rX, recs[it - 1]["rX"]), (k, it)
        if flavour == "bounds":
            difs = np.array([r["dif"] for r in recs], dt)
            assert same_bytes(Dif[:it], difs[:it]), (k, it, Dif[:it], difs[:it])
            assert in_box(p, rX), (k, it)
    # CP_itMax = 0: initialize() alone (bounds: the one-component value projected on the box)
    Cv, rX, it, Obj, Dif, Time = entry(flavour, p, CP_itMax=0)
    assert it == 0 and not Cv.any() and same_bytes(rX, rX0)
    if flavour == "bounds":
        assert in_box(p, rX)
    # the preAt rule (l1 :671, bounds :648) from the twin's own records, PFDR_it
    # from the call before
    taken, pit = [], p["PFDR_itMax"]
    for r in recs:
        if r["preAt"] is None:
            continue
        N = p["N"]
        assert r["preAt"] == (N <= 0 or r["rV"] < (2 * N * pit) // (N + pit)), (r["rV"], pit)
        taken.append(r["preAt"])
        pit = r["pfdr_it"]
    if kind == "direct12":
        assert True in taken and False in taken, taken
    if flavour == "l1" and kind == "direct160":
        # premultiplied with a dense A in all iterations but the second, where
        # rV = 109 >= 88 = (2 160 61) // (160 + 61) after a 61-iteration solve: the
        # rule itself sends that one down the direct branch (the reference's run
        # of this problem has the same Cv and CP_it, test_recorded_run_functional)
        assert True in taken, taken
    if kind in ALL_PREAT[flavour]:
        assert taken and all(taken), taken
    if kind == "zero_tol":
        assert full[2] == 3 and len(recs) == 3
    if kind == "tiny_tol":
        assert T.real_eps(dt, p["CP_difTol"]) == dt(1e-9)
    if kind in NO_CUT[flavour]:
        Cv, rX, it, Obj, Dif, Time = full
        assert rX.size == 1 and not Cv.any()
        if flavour != "bounds":
            assert it == 1
        assert Dif[0] == 0 and Obj[1] == Obj[0]
        assert same_bytes(rX, rX0)
        assert recs[0]["activated"] == 0
    if flavour == "duplex" and kind in ("pos_diag", "l1pos_diag"):
        assert np.all(full[1] >= 0) and recs[-1]["rV"] > 1
    if flavour == "bounds":
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
        if kind in ("pinned", "min_eq_max"):
            assert full[1][0] == real(p["lo"])


# ---------------------------- c. against the reference's own recorded run --
def recorded_run_exact(flavour, name):
    """N = 0: Cv, rX and CP_it of the reference's run, exactly"""
    RC = RUN[flavour]
    g = RC.load(name)
    kind, d = name.rsplit("_", 1)
    p, (Cv, rX, it, Obj, Dif, Time) = full_run(flavour, kind, RC.DTYPES[d])
    assert it == g["CP_it"]
    assert np.array_equal(Cv, g["Cv"])
    assert rX.dtype == g["rX"].dtype and np.array_equal(rX, g["rX"])
    if flavour == "bounds":
        assert RC.at_bounds(p, rX) == RC.EXPECT[kind][2:]


def recorded_run_functional(flavour, d, kind):
    """N != 0: L comes from a power iteration that matches the reference's
    (time-seeded) one to 2e-2 only, so rX is not owed bit for bit: CP_it and the
    partition are equal (bounds: Cv itself), and
    |F(GPU) - F(ref f64)| <= max(1e-5, 4 gap_ref) |F(ref f64)| in f64 on the
    f64 problem, gap_ref the relative difference between the reference's own
    f32 and f64 recorded runs.  For A^tA the functional is the premultiplied
    form (F minus 1/2 ||y||^2, negative): the bound is relative to its
    magnitude.  e: the components the reference left at a bound are the bounds
    entry's, exactly on it."""
    RC = RUN[flavour]
    p64 = RC.problem(kind, F64)
    g32, g64 = RC.load(kind + "_f32"), RC.load(kind + "_f64")
    p, (Cv, rX, it, Obj, Dif, Time) = full_run(flavour, kind, RC.DTYPES[d])
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
    # the first run on an MI355X gave the reference's partition and iteration
    # count in all cases: held from then on
    assert it == g["CP_it"] and rX.size == g["rX"].size
    assert relabel_differences(Cv, g["Cv"]) == 0
    if flavour == "bounds":
        print("at lo / hi GPU %s ref %s" % (RC.at_bounds(p, rX), RC.at_bounds(p, g["rX"])))
        assert np.array_equal(Cv, g["Cv"])
        assert in_box(p, rX)
        real = rX.dtype.type
        for b in (real(p["lo"]), real(p["hi"])):
            assert np.array_equal(rX == b, g["rX"] == b), b


# ------------------------------------- d. Obj and Dif against f64, bounded --
def obj_and_dif_at_every_iteration(flavour, kind, dt):
    """Obj[k] against functional(p, x_k) and Dif[k-1] against
    sum (x_k - x_{k-1})^2 / max(sum x_k^2, eps) in f64, x_k the twin's k-th
    iterate (byte-equal to the entry's, test_entry_is_the_twin); the bounds are
    derived in cp_entry.obj_bound / dif_bound.  The constant 1/2 ||y||^2 of the
    premultiplied form cancels in the difference and is left out.  N > 0
    (direct12, direct160), N == 0 and N < 0 (AtA) each occur."""
    p, rX0, recs, full = path_case(flavour, kind, dt)
    check_obj_dif("%s_%s" % (kind, np.dtype(dt).name), p, rX0, recs, full)


def obj_and_dif_on_fixtures(flavour, name):
    c, d = load_case(name)
    p = fixture_problem(flavour, c)
    rX0, recs = twin_run(p)
    check_obj_dif(name, p, rX0, recs, entry(flavour, p))


# --------------- f. optional outputs, argument errors and repeatability, raw --
def optional_outputs_and_repeatability(flavour):
    p = _24x20(flavour, F32, **({"positivity": 1} if flavour == "duplex" else {}))
    st, Cv, rX, it = raw(flavour, p)
    assert st == 0 and 1 <= it <= p["CP_itMax"]
    if flavour == "duplex":
        assert rX.size > 1
    st, Cv2, rX2, it2 = raw(flavour, p)  # two runs, the same bytes
    assert st == 0 and it2 == it and same_bytes(Cv2, Cv) and same_bytes(rX2, rX)
    for off in ({"Obj": False}, {"Dif": False}, {"Time": False}, {"CP_it": False},
                {"Obj": False, "Dif": False, "Time": False, "CP_it": False}):
        st, Cv2, rX2, it2 = raw(flavour, p, **off)
        assert st == 0, off
        assert same_bytes(Cv2, Cv) and same_bytes(rX2, rX), off
        if off.get("CP_it", True):
            assert it2 == it
    # Dif == NULL and CP_difTol == 0: nothing is tracked, the run goes to CP_itMax
    st, Cv0, rX0, it0 = raw(flavour, p, Dif=False, CP_difTol=0.0, CP_itMax=3)
    assert st == 0 and it0 == 3
    st, Cv1, rX1, it1 = raw(flavour, p, CP_difTol=0.0, CP_itMax=3)
    assert st == 0 and it1 == 3 and same_bytes(Cv0, Cv1) and same_bytes(rX0, rX1)
    if flavour == "bounds":  # a dense problem too
        q = cp_bounds_run_cases.problem("direct12", F32)
        a = raw(flavour, q, CP_itMax=3)
        b = raw(flavour, q, CP_itMax=3, Obj=False, Dif=False, Time=False)
        assert a[0] == 0 and b[0] == 0 and same_bytes(a[1], b[1]) and same_bytes(a[2], b[2])


def argument_errors(flavour):
    p = _24x20(flavour, F32)
    pA = RUN[flavour].problem("AtA", F32)
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
    ]
    if flavour == "bounds":
        bad += [
            ("min > max", p, dict(lo=0.5, hi=0.25)),
            ("min > max", p, dict(lo=inf, hi=-inf)),
            ("NaN bound", p, dict(lo=float("nan"))),
            ("NaN bound", p, dict(hi=float("nan"))),
        ]
    for what, q, over in bad:
        st, Cv, rX, it = raw(flavour, q, **over)
        msg = pfdr.load().pfdr_last_error().decode()
        assert st == 1, (what, st)  # PFDR_ERR_ARG
        assert msg.startswith({"l1": "pfdr_cp_quadratic_d1_l1_f32: ",
                               "duplex": "pfdr_cp_quadratic_d1_l1_duplex_f32: ",
                               "bounds": "pfdr_cp_quadratic_d1_bounds_f32: "}[flavour]), (what, msg)
    if flavour == "bounds":  # missing output pointers
        fn = pfdr.load().pfdr_cp_quadratic_d1_bounds_f32
        Y = np.ascontiguousarray(p["Y"], F32)
        Cv, rX, rV = np.zeros(p["V"], np.int32), np.zeros(p["V"], F32), C.c_int(0)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        for outs in ((None, vp(Cv), vp(rX)), (C.byref(rV), None, vp(rX)),
                     (C.byref(rV), vp(Cv), None)):
            st = fn(C.c_int(p["V"]), C.c_int(0), C.c_int(0), outs[0], outs[1], outs[2], vp(Y),
                    None, None, None, None, C.c_float(-1), C.c_float(1), C.c_float(1e-3),
                    C.c_int(2), None, C.c_float(1.5), C.c_float(1e-3), C.c_float(0),
                    C.c_float(1e-4), C.c_int(100), None, None, None, C.c_int(0))
            assert st == 1
    # the library is still usable
    st, Cv, rX, it = raw(flavour, p)
    assert st == 0 and it >= 1 and rX.size == Cv.max() + 1
    if flavour == "bounds":  # min == max is valid
        st, Cv, rX, it = raw(flavour, p, lo=0.25, hi=0.25)
        assert st == 0 and rX.size == 1 and rX[0] == F32(0.25)


# ------------------------------------------------------------ g. the stats --
def stats(flavour, kind):
    """duplex and bounds: the l1 entry keeps no record"""
    assert flavour in ("duplex", "bounds"), "the l1 entry has no stats call"
    p = RUN[flavour].problem(kind, F32)
    name = {"duplex": "cp_quadratic_d1_l1_duplex_stats",
            "bounds": "cp_quadratic_d1_bounds_stats"}[flavour]
    get_stats = getattr(pfdr.Lib(), name)
    Cv, rX, it, Obj, Dif, Time = entry(flavour, p)
    s = get_stats()
    phases = [s[k] for k in ("gradient", "cuts", "graph", "pfdr", "sums")]
    assert all(x >= 0 for x in phases) and s["total"] > 0
    assert sum(phases) <= s["total"]
    assert Time[it] <= s["total"]
    if flavour == "duplex":
        assert s["n_cuts"] == it  # one two-layer cut per iteration run
        assert s["rounds"] >= 0 and s["relabels"] >= it
    else:
        # every iteration reaches the cut: one cut without a bound, two with
        assert s["n_cuts"] == it * (1 if kind == "free_diag" else 2)
        assert s["rounds"] >= 0 and s["relabels"] >= 0
    if kind == "nothing":
        assert s["pfdr_it"] == 0 and s["pfdr"] == 0
    else:
        assert s["pfdr_it"] > 0 and s["pfdr"] > 0 and s["rounds"] > 0
    if flavour == "duplex":  # the l1 entry leaves this thread's duplex record alone
        entry("l1", p, CP_itMax=1)
        assert get_stats() == s
    # either output may be NULL
    raw_fn = getattr(pfdr.load(), "pfdr_" + name)
    cnt = np.zeros(4, np.int64)
    assert raw_fn(None, None) == 0
    assert raw_fn(None, C.c_void_p(cnt.ctypes.data)) == 0
    assert cnt.tolist() == [s["n_cuts"], s["rounds"], s["relabels"], s["pfdr_it"]]


# ------------------------------------------------- h. the MEX-named front ends --
PAR = (1e-4, 4, 1.5, 1e-3, 0.0, 1e-5, 2000)  # CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax


def _own(flavour, p, **over):
    """the flavour's own arguments of its front ends, after La_d1"""
    q = dict(p, **over)
    return ((q["lo"], q["hi"]),) if flavour == "bounds" else (q["La_l1"], q["positivity"])


def mex_quadratic(flavour):
    """duplex and bounds: the l1 driver has no MEX-named front end here"""
    assert flavour in ("duplex", "bounds"), "no MEX-named front end of the l1 driver"
    front = {"duplex": pfdr.CP_PFDR_graph_quadratic_d1_l1_duplex,
             "bounds": pfdr.CP_PFDR_graph_quadratic_d1_bounds}[flavour]
    p = RUN[flavour].problem("direct12", F32)
    A = np.asarray(p["A"]).reshape(p["V"], p["N"]).T  # N-by-V
    a = (p["Y"], A, p["Eu"], p["Ev"], p["La_d1"]) + _own(flavour, p, positivity=0) + PAR
    got = front(*a, time=True, obj=True, dif=True)
    Obj, wObj = _same_result(got, entry(flavour, p, CP_itMax=PAR[1]), PAR[1])
    assert same_bytes(Obj, wObj)
    Cv, rX, it, Time, Obj, Dif = front(*a)
    assert Time is None and Obj is None and Dif is None and same_bytes(rX, got[1])


def mex_l22(flavour):
    """duplex and bounds, as mex_quadratic"""
    assert flavour in ("duplex", "bounds"), "no MEX-named front end of the l1 driver"
    front = {"duplex": pfdr.CP_PFDR_graph_l22_d1_l1_duplex,
             "bounds": pfdr.CP_PFDR_graph_l22_d1_bounds}[flavour]
    p = P.problem(flavour, "identity", F32, nx=24, ny=18,
                  **({"positivity": 1} if flavour == "duplex" else {}))
    V = p["V"]
    w = (0.5 + np.arange(V) % 4 / 4.0).astype(F32)
    y = np.asarray(p["Y"], F32)
    got = front(y, w, p["Eu"], p["Ev"], p["La_d1"], *_own(flavour, p), *PAR, time=True, obj=True,
                dif=True)
    q = dict(p, Y=(w * y).astype(F32), A=w)
    want = entry(flavour, q, CP_itMax=PAR[1])
    Obj, wObj = _same_result(got, want, PAR[1])
    it = got[2]
    y2 = float(np.sum(w.astype(F64) * y * y)) / 2.0
    expect = wObj.copy()
    expect[: it + 1] += y2
    assert same_bytes(Obj, expect)
    # a scalar La_l2: no weights, the identity; duplex: a scalar La_l1, no l1 term
    got1 = front(y, 1.0, p["Eu"], p["Ev"], p["La_d1"], *_own(flavour, p, La_l1=0.0), *PAR)
    want1 = entry(flavour, dict(p, La_l1=None), CP_itMax=PAR[1])
    assert got1[2] == want1[2] and same_bytes(got1[0], want1[0]) and same_bytes(got1[1], want1[1])
