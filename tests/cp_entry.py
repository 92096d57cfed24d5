"""TEST INFRASTRUCTURE -- what the tests of the one-call quadratic cut pursuits
share (tests/cp_entry_checks.py and the three entry modules that call it,
tests/test_cut_pursuit_gpu.py, tests/cp_solver_cases.py): the entry of a
flavour ("l1", "duplex", "bounds") over a cp_problems dict, through ``pfdr.Lib`` and raw through ctypes, the
functional in f64, and the derived rounding bounds on Obj and Dif.
"""
import ctypes as C

import numpy as np

import cp_twin as T
from cp_pfdr_graph_d1_amd import pfdr

F32, F64 = np.float32, np.float64
REL = 1e-5  # the project's parity bar
# the iteration fixtures' recorder parameters (oracle.CPStepRef*.step defaults)
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=1000)
# the C entry of a flavour, before its type suffix
SYMBOL = {"l1": "pfdr_cp_quadratic_d1_l1_", "duplex": "pfdr_cp_quadratic_d1_l1_duplex_",
          "bounds": "pfdr_cp_quadratic_d1_bounds_"}


def entry(flavour, p, CP_itMax=None, verbose=0, **over):
    """the flavour's ``Lib`` entry -> (Cv, rX, CP_it, Obj, Dif, Time)"""
    q = dict(p)
    q.update(over)
    L = pfdr.Lib()
    a = (q["V"], q["N"], q["Y"], q["A"], q["Eu"], q["Ev"], q["La_d1"])
    kw = dict(CP_difTol=q["CP_difTol"], CP_itMax=q["CP_itMax"] if CP_itMax is None else CP_itMax,
              rho=q["rho"], condMin=q["condMin"], difRcd=q["difRcd"], difTol=q["PFDR_difTol"],
              itMax=q["PFDR_itMax"], verbose=verbose)
    if flavour == "bounds":
        return L.cp_quadratic_d1_bounds(*a, lo=q["lo"], hi=q["hi"], **kw)
    fn = L.cp_quadratic_d1_l1_duplex if flavour == "duplex" else L.cp_quadratic_d1_l1
    return fn(*a, q["La_l1"], positivity=q["positivity"], **kw)


def raw(flavour, p, Obj=True, Dif=True, Time=True, CP_it=True, **over):
    """the flavour's C entry through ctypes -> (status, Cv, rX, CP_it or None);
    Cv starts at -1 and rX at 7 everywhere: untouched outputs show"""
    q = dict(p)
    q.update(over)
    dt = np.dtype(q["dtype"])
    ct = C.c_float if dt == F32 else C.c_double
    fn = getattr(pfdr.load(), SYMBOL[flavour] + ("f32" if dt == F32 else "f64"))
    V, K = q["V"], max(q["CP_itMax"], 0)
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    Y, A, La, L1 = (arr(q[k], dt) for k in ("Y", "A", "La_d1", "La_l1"))
    Eu, Ev = arr(q["Eu"], np.int32), arr(q["Ev"], np.int32)
    Cv, rX = np.full(max(V, 1), -1, np.int32), np.full(max(V, 1), 7, dt)
    o, d, t = np.zeros(K + 1, dt), np.zeros(max(K, 1), dt), np.zeros(K + 1)
    rV, it = C.c_int(-5), C.c_int(-1)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    own = ((ct(q["lo"]), ct(q["hi"])) if flavour == "bounds"
           else (ptr(L1), C.c_int(q["positivity"])))
    st = fn(C.c_int(V), C.c_int(q["E"]), C.c_int(q["N"]), C.byref(rV), ptr(Cv), ptr(rX), ptr(Y),
            ptr(A), ptr(Eu), ptr(Ev), ptr(La), *own, ct(q["CP_difTol"]), C.c_int(q["CP_itMax"]),
            C.byref(it) if CP_it else None, ct(q["rho"]), ct(q["condMin"]), ct(q["difRcd"]),
            ct(q["PFDR_difTol"]), C.c_int(q["PFDR_itMax"]), ptr(t) if Time else None,
            ptr(o) if Obj else None, ptr(d) if Dif else None, C.c_int(0))
    if st != 0:  # nothing may have been written
        assert rV.value == -5 and it.value == -1
        assert np.all(Cv == -1) and np.all(rX == 7)
        assert not o.any() and not d.any() and not t.any()
        return st, Cv, rX, None
    return st, Cv[:max(V, 0)], rX[:rV.value].copy(), it.value if CP_it else None


def fixture_problem(flavour, c):
    """an iteration fixture's inputs as a cp_problems dict"""
    p = dict(kind=flavour, V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=c["Y"].dtype.type,
             CP_itMax=6, PFDR_itMax=STEP["itMax"], positivity=0, CP_difTol=c["CP_difTol"],
             PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
             difRcd=STEP["difRcd"], Y=c["Y"], A=c["A"], Eu=c["Eu"], Ev=c["Ev"],
             La_d1=c["La_d1"], La_l1=None)
    if flavour == "bounds":
        p.update(lo=c["lo"], hi=c["hi"])
    else:
        p.update(positivity=c["positivity"], La_l1=c["La_l1"])
    return p


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def relabel_differences(a, b):
    return int(np.count_nonzero(T.canonical(a) != T.canonical(b)))


def _same_result(got, want, CP_itMax):
    """a MEX-named front end's (Cv, rX, CP_it, Time, Obj, Dif) against the entry's
    (Cv, rX, CP_it, Obj, Dif, Time) -> the two Obj, which the l22 wrappers shift"""
    Cv, rX, it, Time, Obj, Dif = got
    wCv, wrX, wit, wObj, wDif, wTime = want
    assert it == wit and same_bytes(Cv, wCv) and same_bytes(rX, wrX)
    assert Time is not None and Time.size == CP_itMax + 1
    assert same_bytes(Dif, wDif)
    return Obj, wObj


# --------------------------------------------------- the functional in f64 --
def functional(p, x):
    """F(x) = 1/2 ||y - A x||^2 + sum_E w |x_u - x_v| + sum_V la |x_v| in f64, in the
    form the driver's Obj uses: for N <= 0 the premultiplied one, 1/2 <x, AtA x> -
    <x, Aty> (F minus the constant 1/2 ||y||^2)"""
    x = np.asarray(x, np.float64)
    Y = np.asarray(p["Y"], np.float64)
    V, N = p["V"], p["N"]
    if N > 0:
        A = np.asarray(p["A"], np.float64).reshape(V, N).T  # column major N-by-V
        f = 0.5 * np.sum((Y - A @ x) ** 2)
    elif N < 0:
        AA = np.asarray(p["A"], np.float64).reshape(V, V)
        f = 0.5 * x @ (AA @ x) - x @ Y
    else:
        a = np.ones(V) if p["A"] is None else np.asarray(p["A"], np.float64)
        f = np.sum(x * (0.5 * a * x - Y))
    f += np.sum(np.asarray(p["La_d1"], np.float64) * np.abs(x[p["Eu"]] - x[p["Ev"]]))
    if p["La_l1"] is not None:
        f += np.sum(np.asarray(p["La_l1"], np.float64) * np.abs(x))
    return float(f)


def constant(p):
    """1/2 ||y||^2, the term the premultiplied form of N = 0 lacks (the MEX
    wrappers add it): Y = A^t y and the diagonal a of A^tA give y^2 = Y^2 / a"""
    if p["N"] != 0:
        return 0.0
    Y = np.asarray(p["Y"], np.float64)
    a = np.ones(p["V"]) if p["A"] is None else np.asarray(p["A"], np.float64)
    return float(0.5 * np.sum(Y * Y / a))


# --------------------------------------- Obj and Dif against f64, bounded --
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
    The f64 yardstick obeys the same bound with u = 2^-53; callers add it.

    The bounds flavour forms the same sums in the same order -- the
    one-component value from V-term sums (rY, rAA; for N > 0 through the column
    sums rA), 1/2 sum R^2 with R = Y - sum_rv rA x, sum_rv x (1/2 rAA x - rY) or
    its full-matrix form, sum_re rLa |x_ru - x_rv| -- without an l1 term (its
    bound is then 0), and Obj = quad + d1 costs one rounding of the partial sums
    where two are counted here.  The projection of the one-component value onto
    the box is exact (it returns min, max or the value), and F is evaluated at
    the projected value on both sides: the bound holds there term for term."""
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
