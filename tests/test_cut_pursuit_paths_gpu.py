"""The one-call cut pursuit (pfdr_cp_quadratic_d1_l1, csrc/pfdr_cutpursuit.hip)
pinned on every path of its loop.

a. N = 0: Cv, rX and CP_it equal the reference's recorded iterations
   (tests/golden/cp_*.npz) bit for bit, for every truncation CP_itMax = 1..6.
b. Entry against the step-composed twin (tests/cp_twin.py over the library's
   own per-step API): Cv, rX, CP_it byte-identical for every truncation, on the
   direct branch (preAt == 0), the premultiplied dense one, A^tA given,
   positivity without l1, CP_difTol below machine eps, CP_difTol == 0, a
   problem with nothing to cut, E == 0 and V == 1.
c. Obj[k] and Dif[k] at every iteration against f64, within a derived
   rounding bound (``obj_bound`` / ``dif_bound`` below).
d. Dense and A^tA runs against the reference's own recorded run
   (tests/golden/cp_run/): exact for N = 0, a two-sided bound on the
   functional otherwise.
e. Optional outputs (NULL) and argument errors through ctypes.
"""
import ctypes as C

import numpy as np
import pytest

import cp_problems as P
import cp_run_cases as RC
import cp_twin as T
from cp_pfdr_graph_d1_amd import pfdr
from test_cp_graph_oracle import NAMES, load_case
from test_cut_pursuit_gpu import constant, functional

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
REL = 1e-5  # the project's parity bar
# the iteration fixtures' recorder parameters (oracle.CPStepRef.step defaults)
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=1000)


def entry(p, CP_itMax=None, **over):
    q = dict(p)
    q.update(over)
    return pfdr.Lib().cp_quadratic_d1_l1(
        q["V"], q["N"], q["Y"], q["A"], q["Eu"], q["Ev"], q["La_d1"], q["La_l1"],
        positivity=q["positivity"], CP_difTol=q["CP_difTol"],
        CP_itMax=q["CP_itMax"] if CP_itMax is None else CP_itMax, rho=q["rho"],
        condMin=q["condMin"], difRcd=q["difRcd"], difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"])


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fixture_problem(c):
    """an iteration fixture's inputs as a cp_problems dict"""
    dt = c["Y"].dtype.type
    return dict(kind="l1", V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=dt, CP_itMax=6,
                PFDR_itMax=STEP["itMax"], positivity=c["positivity"], CP_difTol=c["CP_difTol"],
                PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
                difRcd=STEP["difRcd"], Y=c["Y"], A=c["A"], Eu=c["Eu"], Ev=c["Ev"],
                La_d1=c["La_d1"], La_l1=c["La_l1"])


# ------------------------------------------ a. exact against the reference --
@pytest.mark.parametrize("name", NAMES)
def test_entry_is_the_reference_run(gpu_lib, name):
    """N = 0: every cut returns the reference's segments, PFDR is
    bit-exact in the graph modes and L is rAA itself, so the entry owes the
    reference's Cv, rX and CP_it exactly.  tests/test_cp_twin_cpu.py checks that
    the recorded warm-restart chain is the reference's one-call run."""
    c, d = load_case(name)
    p = fixture_problem(c)
    tol2 = c["Y"].dtype.type(c["CP_difTol"]) ** 2
    for k in range(1, int(d["meta_steps"]) + 1):
        Cv, rX, it, Obj, Dif, Time = entry(p, CP_itMax=k)
        assert 1 <= it <= k
        assert it == k or Dif[it - 1] < tol2, (k, it, Dif[:it])
        assert np.array_equal(Cv, d["k%d_out_Cv" % (it - 1)]), (k, it)
        want = d["k%d_out_rX" % (it - 1)]
        assert rX.dtype == want.dtype and np.array_equal(rX, want), (k, it)


# ------------------------------------------------ b. entry against the twin --
def _small(dt, V):
    """V vertices without an edge"""
    z = np.zeros(0, np.int32)
    y = (np.arange(V) % 3 - 0.75).astype(dt)
    return dict(kind="l1", V=V, E=0, N=0, K=0, dtype=dt, CP_itMax=3, PFDR_itMax=2000,
                positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3,
                difRcd=0.0, Y=y, A=None, Eu=z, Ev=z, La_d1=np.zeros(0, dt), La_l1=None)


def _l1_24x20(dt, **over):
    return P.problem("l1", "diag", dt, nx=24, ny=20, **over)


PATHS = {
    "direct12": lambda dt: RC.problem("direct12", dt),
    "direct160": lambda dt: RC.problem("direct160", dt),
    "AtA": lambda dt: RC.problem("AtA", dt),
    "pos_diag": lambda dt: RC.problem("pos_diag", dt),
    "tiny_tol": lambda dt: _l1_24x20(dt, CP_difTol=1e-9, CP_itMax=4),
    "zero_tol": lambda dt: _l1_24x20(dt, CP_difTol=0.0, CP_itMax=3),
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
        t = T.gpu_twin(p)
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
    for k in range(1, K + 1):
        Cv, rX, it, Obj, Dif, Time = full if k == K else entry(p, CP_itMax=k)
        assert it == min(k, len(recs)), (k, it, len(recs))
        assert same_bytes(Cv, recs[it - 1]["Cv"]), (k, it)
        assert same_bytes(rX, recs[it - 1]["rX"]), (k, it)
    # CP_itMax = 0: initialize() alone
    Cv, rX, it, Obj, Dif, Time = entry(p, CP_itMax=0)
    assert it == 0 and not Cv.any() and same_bytes(rX, rX0)
    # the preAt rule (:671) from the twin's own records, PFDR_it from the call before
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
    if kind == "direct160":
        # premultiplied with a dense A in all iterations but the second, where
        # rV = 109 >= 88 = (2 160 61) // (160 + 61) after a 61-iteration solve: the
        # rule itself sends that one down the direct branch (the reference's run
        # of this problem has the same Cv and CP_it, test_recorded_run_functional)
        assert True in taken, taken
    if kind in ("AtA", "pos_diag"):
        assert taken and all(taken), taken
    if kind == "zero_tol":
        assert full[2] == 3 and len(recs) == 3
    if kind == "tiny_tol":
        assert T.real_eps(dt, p["CP_difTol"]) == dt(1e-9)
    if kind in ("nothing", "E0_V5", "E0_V1"):
        Cv, rX, it, Obj, Dif, Time = full
        assert rX.size == 1 and it == 1 and not Cv.any()
        assert Dif[0] == 0 and Obj[1] == Obj[0]
        assert same_bytes(rX, rX0)
        assert recs[0]["activated"] == 0


# ------------------------------------- c. Obj and Dif against f64, bounded --
def gamma(n, u):
    return n * u / (1 - n * u)


def obj_bound(p, Cv, rX, u):
    """Bound on |Obj - F(x)|, x = rX[Cv], for unit roundoff u.

    The driver adds its terms one by one; any summation of n terms t obeys
    |fl(sum t) - sum t| <= gamma_{n-1} sum |t|, gamma_n = n u / (1 - n u), and
    a chain of k roundings on a term costs at most gamma_k of it.  Count the
    roundings each ORIGINAL term of F goes through (c a component, |c| its
    size, rV components, so |c| + rV <= V + 1):

    * N = 0:  sum_rv x (1/2 rAA x - rY), rAA = sum_c a_v, rY = sum_c Y_v:
      |c| - 1 additions, two products, the difference, rV additions:
      <= V + 3 roundings on  1/2 a_v x_v^2  and on  Y_v x_v.
    * N < 0:  sum_ru x_ru (1/2 b_ru - rY_ru), b_ru = sum_rv rAA[ru, rv] x_rv,
      rAA[ru, rv] a sum of |c_u||c_v| entries: |c_u||c_v| - 1 additions, one
      product, rV additions (the inner row product), the difference, one
      product, rV additions (the outer sum): <= m = max|c|^2 + 2 rV + 2 on
      1/2 A_uv x_u x_v;  Y_v x_v as above.
    * N > 0:  1/2 sum_n R_n^2,  R_n = Y_n - sum_rv rA[n, rv] x_rv,  rA a sum of
      |c| columns: A_nv x_v goes through <= V + 1 roundings, the difference
      one more:  |R^_n - R_n| <= d_n = u |R_n| + gamma_{V+2} s_n,
      s_n = sum_v |A_nv x_v|.  Squares and their N-term sum: gamma_{N+1}.  So
      |1/2 sum R^^2 - 1/2 sum R^2| <= 1/2 [gamma_{N+1} sum (|R_n| + d_n)^2
                                           + sum d_n (2 |R_n| + d_n)].
    * d1:  sum_re rLa |x_ru - x_rv|, rLa a sum of the edges between two
      components (eps self-loops multiply a zero difference): the difference,
      the edge sum, the product, <= rE additions: <= E + V + 2 roundings on
      La_e |x_u - x_v|.
    * l1:  sum_rv rL1 |x_rv|: <= V + 1 roundings on la_v |x_v|.
    * Obj = (quad + d1) + l1: two more roundings of the partial sums.

    Underflow is not counted: every term here is far above the smallest normal.
    The f64 yardstick obeys the same bound with u = 2^-53; callers add it."""
    V, N, E = p["V"], p["N"], p["E"]
    x = np.asarray(rX, F64)[Cv]
    Y = np.asarray(p["Y"], F64)
    rV = int(Cv.max()) + 1
    if N > 0:
        A = np.asarray(p["A"], F64).reshape(V, N).T
        R = np.abs(Y - A @ x)
        s = np.abs(A) @ np.abs(x)
        d = u * R + gamma(V + 2, u) * s
        quad = 0.5 * (gamma(N + 1, u) * np.sum((R + d) ** 2) + np.sum(d * (2 * R + d)))
        mag = 0.5 * np.sum(R * R)
    elif N < 0:
        AA = np.abs(np.asarray(p["A"], F64).reshape(V, V))
        m = int(np.bincount(Cv).max()) ** 2 + 2 * rV + 2
        ax = np.abs(x)
        t1, t2 = 0.5 * ax @ (AA @ ax), np.sum(np.abs(Y * x))
        quad = gamma(m, u) * t1 + gamma(V + 3, u) * t2
        mag = t1 + t2
    else:
        a = np.ones(V) if p["A"] is None else np.asarray(p["A"], F64)
        mag = np.sum(0.5 * a * x * x + np.abs(Y * x))
        quad = gamma(V + 3, u) * mag
    d1 = np.sum(np.asarray(p["La_d1"], F64) * np.abs(x[p["Eu"]] - x[p["Ev"]])) if E else 0.0
    l1 = 0.0 if p["La_l1"] is None else np.sum(np.asarray(p["La_l1"], F64) * np.abs(x))
    return float(quad + gamma(E + V + 2, u) * d1 + gamma(V + 1, u) * l1
                 + gamma(2, u) * (mag + d1 + l1))


def dif_f64(x, x_, eps):
    x, x_ = np.asarray(x, F64), np.asarray(x_, F64)
    return float(np.sum((x - x_) ** 2) / max(np.sum(x * x), eps))


def dif_bound(V, dif, denom, u, tiny):
    """dif = sum (x' - x)^2 / c, c = sum x^2 (or eps): every term of either sum
    is positive, so each sum is relatively exact to gamma_{V+2} (difference,
    square, V additions) resp. gamma_{V+1}, the quotient adds u:
    (1 + gamma_{V+2})(1 + u) / (1 - gamma_{V+1}) - 1 relative; a square that
    underflows loses at most the smallest normal ``tiny``, V of them."""
    rel = (1 + gamma(V + 2, u)) * (1 + u) / (1 - gamma(V + 1, u)) - 1
    return rel * dif + V * tiny / denom


def check_obj_dif(tag, p, rX0, recs, out):
    Cv, rX, it, Obj, Dif, Time = out
    dt = np.dtype(p["dtype"])
    u, u64 = float(np.finfo(dt).eps) / 2, 2.0 ** -53
    tiny = float(np.finfo(dt).tiny)
    eps = float(T.real_eps(dt, p["CP_difTol"]))
    tol2 = dt.type(p["CP_difTol"]) ** 2
    # CP_it from the returned arrays alone
    first = next((k for k in range(1, p["CP_itMax"] + 1) if Dif[k - 1] < tol2), p["CP_itMax"])
    assert it == first, (it, first, Dif)
    assert it == len(recs)
    states = [(np.zeros(p["V"], np.int32), rX0)] + [(r["Cv"], r["rX"]) for r in recs]
    worst_o = worst_d = 0.0
    for k, (cv, rx) in enumerate(states):
        x = np.asarray(rx, F64)[cv]
        F = functional(p, x)
        bo = obj_bound(p, cv, rx, u) + obj_bound(p, cv, rx, u64)
        eo = abs(float(Obj[k]) - F)
        scale = abs(F + constant(p)) or 1.0  # one vertex: F + 1/2 y^2 = 0
        print("%s Obj[%d] %.9g F %.9g |err| %.3e bound %.3e (rel %.2e / %.2e)" % (
            tag, k, Obj[k], F, eo, bo, eo / scale, bo / scale))
        assert eo <= bo, (tag, k, eo, bo)
        worst_o = max(worst_o, eo / bo if bo else 0.0)
        if k == 0:
            continue
        x_ = np.asarray(states[k - 1][1], F64)[states[k - 1][0]]
        want = dif_f64(x, x_, eps)
        denom = max(float(np.sum(x * x)), eps)
        bd = dif_bound(p["V"], want, denom, u, tiny) + dif_bound(p["V"], want, denom, u64, 0.0)
        ed = abs(float(Dif[k - 1]) - want)
        print("%s Dif[%d] %.9g f64 %.9g |err| %.3e bound %.3e" % (tag, k - 1, Dif[k - 1], want,
                                                                 ed, bd))
        assert ed <= bd, (tag, k, ed, bd)
        worst_d = max(worst_d, ed / bd if bd else 0.0)
    print("%s worst |err| / bound: Obj %.3f Dif %.3f" % (tag, worst_o, worst_d))


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_obj_and_dif_at_every_iteration(gpu_lib, kind, dt):
    """Obj[k] against functional(p, x_k) and Dif[k-1] against
    sum (x_k - x_{k-1})^2 / max(sum x_k^2, eps) in f64, x_k the twin's k-th
    iterate (byte-equal to the entry's, test_entry_is_the_twin); the bounds are
    derived in obj_bound / dif_bound.  The constant 1/2 ||y||^2 of the
    premultiplied form cancels in the difference and is left out.  N > 0
    (direct12, direct160), N == 0 and N < 0 (AtA) each occur."""
    p, rX0, recs, full = path_case(kind, dt)
    check_obj_dif("%s_%s" % (kind, np.dtype(dt).name), p, rX0, recs, full)


@pytest.mark.parametrize("name", ["cp_grid2d_l1_f32", "cp_knn_diag_l1pos_f64"])
def test_obj_and_dif_on_fixtures(gpu_lib, name):
    c, d = load_case(name)
    p = fixture_problem(c)
    t = T.gpu_twin(p)
    rX0, recs = t.run(p["CP_itMax"])
    t.b.close()
    check_obj_dif(name, p, rX0, recs, entry(p))


# ---------------------------- d. against the reference's own recorded run --
def relabel_differences(a, b):
    return int(np.count_nonzero(T.canonical(a) != T.canonical(b)))


@pytest.mark.parametrize("name", [n for n in RC.NAMES if n.startswith(("pos_diag", "nothing"))])
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
    (time-seeded) one to 2e-2 only, so rX is not owed bit for bit:
    |F(GPU) - F(ref f64)| <= max(1e-5, 4 gap_ref) |F(ref f64)| in f64 on the
    f64 problem, gap_ref the relative difference between the reference's own
    f32 and f64 recorded runs.  For A^tA the functional is the premultiplied
    form (F minus 1/2 ||y||^2, negative): the bound is relative to its
    magnitude."""
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
    # the first run on an MI355X gave the reference's partition and iteration
    # count in all six cases: held from then on
    assert it == g["CP_it"] and rX.size == g["rX"].size
    assert relabel_differences(Cv, g["Cv"]) == 0


# --------------------------- e. optional outputs and argument errors, raw --
def raw(p, Obj=True, Dif=True, Time=True, CP_it=True, **over):
    """pfdr_cp_quadratic_d1_l1_* through ctypes -> (status, Cv, rX, CP_it or None)"""
    q = dict(p)
    q.update(over)
    dt = np.dtype(q["dtype"])
    ct = C.c_float if dt == F32 else C.c_double
    fn = getattr(pfdr.load(), "pfdr_cp_quadratic_d1_l1_" + ("f32" if dt == F32 else "f64"))
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


def test_optional_outputs(gpu_lib):
    p = P.problem("l1", "diag", F32, nx=24, ny=20)
    st, Cv, rX, it = raw(p)
    assert st == 0 and 1 <= it <= p["CP_itMax"]
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
    p = P.problem("l1", "diag", F32, nx=24, ny=20)
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
        assert msg.startswith("pfdr_cp_quadratic_d1_l1_f32: "), (what, msg)
    # the library is still usable
    st, Cv, rX, it = raw(p)
    assert st == 0 and it >= 1 and rX.size == Cv.max() + 1
