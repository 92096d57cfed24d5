"""The simplex driver's one-call cut pursuit (pfdr_cp_loss_d1_simplex,
csrc/pfdr_cutpursuit_simplex.hip) pinned on every path of its loop.

a. Cv, rP and CP_it equal the reference's recorded iterations
   (tests/golden/cp_simplex_*.npz) bit for bit, for every truncation
   CP_itMax = 1..6 of the ten fixtures (tests/test_cp_simplex_twin_cpu.py checks
   that the recorded warm-restart chain is the reference's one-call run).
b. Entry against the step-composed twin (tests/cp_simplex_twin.py over the
   library's own per-step API): Cv, rP, CP_it and Dif byte-identical for every
   truncation CP_itMax = 0..k, on every path of the loop (``PATHS``).
c. The reference's own recorded continuous runs (tests/golden/cp_simplex_run/):
   Cv, rP and CP_it exactly.
d. Obj[k], Obj[0] included, against the functional in f64 at the entry's own
   (Cv, rP), within a derived rounding bound (``obj_bound``).
e. Optional outputs (NULL) and argument errors through ctypes.
f. The Python front-end; determinism.
"""
import ctypes as C

import numpy as np
import pytest

import cp_problems as P
import cp_simplex_run_cases as SR
import cp_simplex_twin as ST
from cp_fixtures import SNAMES, load_case
from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import grid_graph, uniform

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
# the iteration fixtures' recorder parameters (oracle.CPStepRefSimplex.step defaults)
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-3, itMax=1000)


def entry(p, CP_itMax=None, **over):
    """-> (Cv, rP, CP_it, Obj, Dif, Time)"""
    q = dict(p)
    q.update(over)
    return pfdr.Lib().cp_loss_d1_simplex(
        q["K"], q["Y"], q["Eu"], q["Ev"], q["La_d1"], al=q["al"], CP_difTol=q["CP_difTol"],
        CP_itMax=q["CP_itMax"] if CP_itMax is None else CP_itMax, rho=q["rho"],
        condMin=q["condMin"], difRcd=q["difRcd"], difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"])


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fixture_problem(c, CP_difTol=None):
    """an iteration fixture's inputs as a cp_problems dict"""
    dt = c["Q"].dtype.type
    return dict(kind="simplex", V=c["Q"].size // c["K"], E=c["Eu"].size, N=0, K=c["K"], dtype=dt,
                CP_itMax=6, PFDR_itMax=STEP["itMax"],
                CP_difTol=c["CP_difTol"] if CP_difTol is None else CP_difTol,
                PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
                difRcd=STEP["difRcd"], al=c["al"], Y=c["Q"], Eu=c["Eu"], Ev=c["Ev"],
                La_d1=c["La_d1"])


# ------------------------------------------ a. exact against the reference --
def test_ten_fixtures_of_six_steps():
    assert len(SNAMES) == 10
    assert sum(int(load_case(n)[1]["meta_steps"]) for n in SNAMES) == 60


@pytest.mark.parametrize("name", SNAMES)
def test_entry_is_the_reference_run(gpu_lib, name):
    """Every cut returns the reference's segments and PFDR is bit-exact on
    these reduced problems, so the entry owes the reference's Cv,
    rP and CP_it exactly.  CP_difTol is the smallest positive normal: positive,
    so eps stays the machine epsilon the fixtures were recorded with, and the
    run stops early only on an evolution of exactly zero."""
    c, d = load_case(name)
    tiny = float(np.finfo(c["Q"].dtype).tiny)
    p = fixture_problem(c, CP_difTol=tiny)
    K = c["K"]
    for n in range(1, int(d["meta_steps"]) + 1):
        Cv, rP, it, Obj, Dif, Time = entry(p, CP_itMax=n)
        assert 1 <= it <= n
        assert it == n or Dif[it - 1] == 0, (n, it, Dif[:it])
        want_Cv, want = d["k%d_out_Cv" % (it - 1)], d["k%d_out_rP" % (it - 1)]
        assert rP.size == want.size and rP.size == K * (int(Cv.max()) + 1), (n, it)
        assert same_bytes(Cv, want_Cv), (n, it)
        assert same_bytes(rP, want), (n, it)


# ------------------------------------------------ b. entry against the twin --
def sx_problem(dt, K, nx, ny, al, lab=None, noise=0.2, seed=7, **over):
    """a cp_problems-style simplex problem with K labels on an nx x ny grid;
    ``lab(x, y) -> label`` of every vertex (default: K vertical bands)"""
    V = nx * ny
    Eu, Ev = grid_graph((nx, ny), 4)
    Eu, Ev = Eu.astype(np.int32), Ev.astype(np.int32)
    v = np.arange(V)
    lb = (v % nx) * K // nx if lab is None else lab(v % nx, v // nx)
    Q = noise * (2 * uniform(seed + 1, np.arange(K * V)).reshape(V, K))
    Q[v, lb] += 1.0
    Q /= Q.sum(1, keepdims=True)
    p = dict(kind="simplex", V=V, E=Eu.size, N=0, K=K, dtype=dt, CP_itMax=4, PFDR_itMax=2000,
             CP_difTol=1e-4, PFDR_difTol=1e-4, rho=1.0, condMin=0.1, difRcd=0.0, al=al,
             Y=Q.astype(dt).ravel(), Eu=Eu, Ev=Ev, La_d1=np.full(Eu.size, 0.1, dt))
    p.update(over)
    return p


def _no_edges(dt, V):
    z = np.zeros(0, np.int32)
    Q = 0.1 + uniform(3, np.arange(3 * V)).reshape(V, 3)
    Q /= Q.sum(1, keepdims=True)
    return dict(kind="simplex", V=V, E=0, N=0, K=3, dtype=dt, CP_itMax=3, PFDR_itMax=2000,
                CP_difTol=1e-4, PFDR_difTol=1e-4, rho=1.0, condMin=0.1, difRcd=0.0, al=0.1,
                Y=Q.astype(dt).ravel(), Eu=z, Ev=z, La_d1=np.zeros(0, dt))


def _constant(dt):
    p = sx_problem(dt, 3, 8, 6, 1.0)
    p["Y"] = np.tile(np.array([0.5, 0.25, 0.25], dt), p["V"])
    return p


def _disconnected(dt):
    c, _ = load_case("cp_simplex_disconnected_" + ("f32" if dt is F32 else "f64"))
    p = fixture_problem(c)
    p["CP_itMax"] = 4
    return p


def _simplex_24x18(dt, **over):
    over.setdefault("CP_itMax", 4)
    return P.problem("simplex", None, dt, nx=24, ny=18, **over)


PATHS = {
    # the label-count evolution; eps is the machine epsilon (2 / V > 0)
    "labels": lambda dt: P.problem("simplex", None, dt, nx=24, ny=20, CP_difTol=2.0, CP_itMax=4),
    # PFDR's own label-count stopping rule, its tolerance divided by V in eps
    "pfdr_tol3": lambda dt: _simplex_24x18(dt, PFDR_difTol=3.0, CP_itMax=3),
    # eps = 0; Dif is requested, so the evolution is tracked and the run goes to CP_itMax
    "zero_tol": lambda dt: _simplex_24x18(dt, CP_difTol=0.0),
    # one expansion per iteration; label 0 the most confident of the one component
    "K2": lambda dt: sx_problem(dt, 2, 16, 12, 0.1, lab=lambda x, y: (x >= 11).astype(int)),
    # seven labels, label 3 the most confident of the one component
    "K7": lambda dt: sx_problem(dt, 7, 21, 12, 0.2, CP_itMax=3,
                                lab=lambda x, y: np.where(x < 9, 3, x * 7 // 21)),
    "linear": lambda dt: _simplex_24x18(dt, al=0.0),
    "quadratic": lambda dt: _simplex_24x18(dt, al=1.0),
    "kl": lambda dt: _simplex_24x18(dt),
    "constant": _constant,
    "disconnected": _disconnected,
    "E0_V5": lambda dt: _no_edges(dt, 5),
    "V1": lambda dt: _no_edges(dt, 1),
}
PATH_IDS = [(k, dt) for k in PATHS for dt in (F32, F64)]
_ids = ["%s_%s" % (k, "f32" if dt is F32 else "f64") for k, dt in PATH_IDS]
_cache = {}


def path_case(kind, dt):
    """-> (problem, twin's rP0, twin's records, the entry's runs for CP_itMax = 0..k)"""
    key = (kind, dt)
    if key not in _cache:
        p = PATHS[kind](dt)
        t = ST.gpu_twin(p)
        rP0, recs = t.run(p["CP_itMax"])
        t.b.close()
        runs = [entry(p, CP_itMax=k) for k in range(p["CP_itMax"] + 1)]
        _cache[key] = (p, rP0, recs, runs)
    return _cache[key]


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_entry_is_the_twin(gpu_lib, kind, dt):
    """Both sides run the same library, so any difference is a wiring
    difference.  The twin goes through the host-memory entries; the driver
    through device memory and a session: the same solver class either way."""
    p, rP0, recs, runs = path_case(kind, dt)
    K, V = p["K"], p["V"]
    print(kind, np.dtype(dt).name, "twin: rV", [r["rV"] for r in recs], "activated",
          [r["activated"] for r in recs], "PFDR it", [r["pfdr_it"] for r in recs], "dif",
          [r["dif"] for r in recs])
    # CP_itMax = 0: initialize() alone
    Cv, rP, it, Obj, Dif, Time = runs[0]
    assert it == 0 and not Cv.any() and same_bytes(rP, rP0)
    difs = np.array([r["dif"] for r in recs], dt)
    for k in range(1, p["CP_itMax"] + 1):
        Cv, rP, it, Obj, Dif, Time = runs[k]
        assert it == min(k, len(recs)), (k, it, len(recs))
        assert same_bytes(Cv, recs[it - 1]["Cv"]), (k, it)
        assert same_bytes(rP, recs[it - 1]["rP"]), (k, it)
        assert same_bytes(Dif[:it], difs[:it]), (k, Dif[:it], difs[:it])
    full = runs[-1]
    eps_m = float(np.finfo(dt).eps)
    eps = ST.simplex_eps(dt, V, p["CP_difTol"], p["PFDR_difTol"])
    if kind == "labels":
        assert eps == eps_m
        assert all(float(r["dif"]) == int(r["dif"]) for r in recs)  # a count
        assert any(r["dif"] > 0 for r in recs)
    if kind == "pfdr_tol3":
        assert eps == eps_m
    if kind == "zero_tol":
        assert eps == 0.0
        assert full[2] == p["CP_itMax"] == len(recs)
    if kind == "K2":
        assert all(len(r["segments"]) == 1 for r in recs)
        assert ST.first_max(rP0, K)[0] == 0 and recs[0]["activated"] > 0
    if kind == "K7":
        assert ST.first_max(rP0, K)[0] == 3
        assert recs[0]["activated"] > 0
    if kind in ("linear", "quadratic", "kl", "disconnected"):
        assert recs[0]["activated"] > 0 and recs[0]["rV"] > 1
    if kind == "disconnected":
        assert recs[0]["rV"] >= 3  # the isolated vertex and two grids
    if kind in ("constant", "E0_V5", "V1"):
        Cv, rP, it, Obj, Dif, Time = full
        assert rP.size == K and it == 1 and not Cv.any()
        assert Dif[0] == 0 and Obj[1] == Obj[0]
        assert same_bytes(rP, rP0)
        assert recs[0]["activated"] == 0


# ------------------------------ c. the reference's recorded continuous runs --
@pytest.mark.parametrize("name", SR.NAMES)
def test_recorded_run_exact(gpu_lib, name):
    """Cv, rP and CP_it of the reference's own continuous run, exactly.  On a
    difference, run tests/cp_simplex_twin.py's twin over both backends to name
    the first iteration and expansion that differ."""
    p = SR.by_name(name)
    g = SR.load(name)
    assert g["hash"] == SR.input_hash(p)
    Cv, rP, it, Obj, Dif, Time = entry(p)
    print(name, "CP_it", it, "ref", g["CP_it"], "rV", rP.size // p["K"], "ref",
          g["rP"].size // p["K"], "Dif", Dif[:it])
    assert it == g["CP_it"]
    assert same_bytes(Cv, g["Cv"])
    assert same_bytes(rP, g["rP"])


# --------------------------------------------- d. Obj against f64, bounded --
def gamma(n, u):
    return n * u / (1 - n * u)


LOG_ULPS = 3.0  # the OpenCL full-profile bound on log; see obj_bound


def functional(p, Cv, rP):
    """-> (F, loss terms t[V, K] or their linear counterpart, d1) in f64 at
    P = rP[Cv]; al as the entry reads it (rounded to the problem's type)"""
    K, V = p["K"], p["V"]
    al = float(np.dtype(p["dtype"]).type(p["al"]))
    Pm = np.asarray(rP, F64).reshape(-1, K)[Cv]
    Q = np.asarray(p["Y"], F64).reshape(V, K)
    if al == 0:
        t = -(Pm * Q)
    elif al == 1:
        t = 0.5 * (Pm - Q) ** 2
    else:
        c = al / K + (1 - al) * Q
        t = c * np.log(c / (al / K + (1 - al) * Pm))
    d1 = 0.0
    if p["E"]:
        d1 = float(np.sum(np.asarray(p["La_d1"], F64)
                          * np.abs(Pm[p["Eu"]] - Pm[p["Ev"]]).sum(1)))
    return float(t.sum()) + d1, t, d1


def obj_bound(p, Cv, rP, u, log_ulps):
    """Bound on |Obj - F(P)|, P = rP[Cv], for unit roundoff u.

    The driver adds its terms one by one; any summation of n terms t obeys
    |fl(sum t) - sum t| <= gamma_{n-1} sum |t|, gamma_n = n u / (1 - n u), and
    a chain of k roundings on a term costs at most gamma_k of it.  Count the
    roundings each ORIGINAL term of F goes through (c a component, |c| its
    size, rV components):

    * linear:  sum over rV K of -(rP rQ), rQ = sum_c Q_v in Vc order: |c| - 1
      additions, the product, rV K additions: <= V + rV K <= V (K + 1)
      roundings on  p_k q_vk.
    * quadratic:  1/2 sum (p - q)^2: the difference (squared: two relative
      errors), the square, V K additions; the halving is exact: gamma_{VK + 3}
      on  1/2 (p - q)^2.
    * smoothed KL:  t = c log(c / d), c = al/K + (1 - al) q, d = al/K + (1 - al) p,
      all positive.  al/K and 1 - al round once each, the product and the sum
      once each: c^ = c (1 + theta_3), d^ = d (1 + theta_3), the quotient once
      more: r^ = r (1 + theta_7), so log r^ = log r + eta, |eta| <= h =
      gamma_7 / (1 - gamma_7).  The device's log: |log^ x - log x| <= log_ulps
      ulp <= 2 log_ulps u |log x|.  LOG_ULPS = 3 is what the OpenCL C
      specification allows log in full profile, the requirement the device
      math library (OCML) is written to; the HIP math API tables quote 1 ulp
      for logf and log, which test_device_log_against_numpy does not see held
      for f32 near x = 1: it measures the device's log against numpy's f64 log
      over the very arguments c / d that occur (1.77 ulp in f32, 1.00 in f64 on
      an MI355X) and holds it to LOG_ULPS.  One rounding for the
      product:
        |t^ - t| <= e = c |log r| (m - 1) + c h m,
        m = (1 + gamma_3)(1 + 2 log_ulps u)(1 + u),
      then V K additions of the computed terms: gamma_{VK} (sum |t| + sum e).
    * d1:  sum_re rLa (sum_k |p_uk - p_vk|), rLa a sum of the edges between two
      components in the reduced graph's visiting order (eps self-loops multiply
      a zero difference): <= E additions, the difference, K additions, the
      product, <= rE <= E + V additions: <= 2 E + V + K + 2 roundings on
      La_e |p_uk - p_vk|.
    * Obj = loss + d1: one more rounding of the two parts (gamma_2 taken).

    Underflow is not counted: every term here is far above the smallest normal.
    The f64 yardstick obeys the same bound with u = 2^-53 and an exact log
    (numpy's, < 1 ulp); callers add it."""
    K, V, E = p["K"], p["V"], p["E"]
    al = float(np.dtype(p["dtype"]).type(p["al"]))
    F, t, d1 = functional(p, Cv, rP)
    mag = float(np.abs(t).sum())
    if al == 0:
        loss = gamma(V * (K + 1), u) * mag
    elif al == 1:
        loss = gamma(V * K + 3, u) * mag
    else:
        Pm = np.asarray(rP, F64).reshape(-1, K)[Cv]
        Q = np.asarray(p["Y"], F64).reshape(V, K)
        c = al / K + (1 - al) * Q
        h = gamma(7, u) / (1 - gamma(7, u))
        m = (1 + gamma(3, u)) * (1 + 2 * log_ulps * u) * (1 + u)
        e = float(np.sum(np.abs(t) * (m - 1) + c * h * m))
        loss = e + gamma(V * K, u) * (mag + e)
    return float(loss + gamma(2 * E + V + K + 2, u) * d1 + gamma(2, u) * (mag + d1))


OBJ_CASES = [("linear", F32), ("quadratic", F32), ("kl", F32), ("kl", F64), ("quadratic", F64),
             ("linear", F64), ("K7", F32), ("disconnected", F64), ("constant", F32),
             ("V1", F64)]


@pytest.mark.parametrize("kind,dt", OBJ_CASES,
                         ids=["%s_%s" % (k, np.dtype(d).name) for k, d in OBJ_CASES])
def test_obj_at_every_iteration(gpu_lib, kind, dt):
    """Obj[k], k = 0..CP_it, against the functional in f64 at the state the
    entry itself returns when stopped at k (the truncated runs are the full
    run's prefixes: their Obj records agree byte for byte)."""
    p, rP0, recs, runs = path_case(kind, dt)
    u, u64 = float(np.finfo(dt).eps) / 2, 2.0 ** -53
    full = runs[-1]
    worst = 0.0
    for k, (Cv, rP, it, Obj, Dif, Time) in enumerate(runs):
        assert same_bytes(Obj[:it + 1], full[3][:it + 1]), k
        F, t, d1 = functional(p, Cv, rP)
        b = obj_bound(p, Cv, rP, u, LOG_ULPS) + obj_bound(p, Cv, rP, u64, 1.0)
        e = abs(float(Obj[it]) - F)
        print("%s_%s Obj[%d] %.9g F %.9g |err| %.3e bound %.3e ratio %.3f" % (
            kind, np.dtype(dt).name, it, Obj[it], F, e, b, e / b if b else 0.0))
        assert np.isfinite(Obj[it]) and e <= b, (kind, k, e, b)
        worst = max(worst, e / b if b else 0.0)
    print("%s_%s worst |err| / bound: %.3f" % (kind, np.dtype(dt).name, worst))


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_device_log_against_numpy(gpu_lib, dt):
    """The margin LOG_ULPS of obj_bound, measured: the device's log as the
    objective kernel's translation unit compiles it (pfdr_debug_device_log)
    against numpy's f64 log of the same rounded arguments, over the ratios
    c / d the KL objective takes its log of in the ``kl`` case."""
    p, rP0, recs, runs = path_case("kl", dt)
    code = pfdr.PFDR_F32 if dt is F32 else pfdr.PFDR_F64
    K, V = p["K"], p["V"]
    real = np.dtype(dt).type
    al = real(p["al"])
    alK, al1 = al / real(K), real(1) - al
    worst = 0.0
    for Cv, rP, it, Obj, Dif, Time in runs:
        c = alK + al1 * np.asarray(p["Y"], dt).reshape(V, K)
        d = alK + al1 * rP.reshape(-1, K)[Cv]
        r = np.ascontiguousarray((c / d).astype(dt).ravel())
        out = np.empty_like(r)
        st = pfdr.load().pfdr_debug_device_log(C.c_int(code), C.c_int64(r.size),
                                               C.c_void_p(r.ctypes.data),
                                               C.c_void_p(out.ctypes.data))
        assert st == 0
        got = out.astype(F64)
        want = np.log(r.astype(F64))
        ulp = np.spacing(np.abs(want).astype(dt)).astype(F64)
        worst = max(worst, float(np.max(np.abs(got - want) / ulp)))
    print("device log %s: worst error %.3f ulp over the kl case's arguments (margin %g)" % (
        np.dtype(dt).name, worst, LOG_ULPS))
    assert worst <= LOG_ULPS


# --------------------------- e. optional outputs and argument errors, raw --
def raw(p, Obj=True, Dif=True, Time=True, CP_it=True, rV=True, Cv=True, rP=True, **over):
    """pfdr_cp_loss_d1_simplex_* through ctypes -> (status, Cv, rP, CP_it or None)"""
    q = dict(p)
    q.update(over)
    dt = np.dtype(q["dtype"])
    ct = C.c_float if dt == F32 else C.c_double
    sfx = "f32" if dt == F32 else "f64"
    fn = getattr(pfdr.load(), "pfdr_cp_loss_d1_simplex_" + sfx)
    V, K, n = q["V"], q["K"], max(q["CP_itMax"], 0)
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    Q, La = arr(q["Y"], dt), arr(q["La_d1"], dt)
    Eu, Ev = arr(q["Eu"], np.int32), arr(q["Ev"], np.int32)
    cv = np.full(max(V, 1), -1, np.int32)
    rp = np.zeros(max(V, 1) * max(K, 1), dt)
    o, d, t = np.zeros(n + 1, dt), np.zeros(max(n, 1), dt), np.zeros(n + 1)
    nrv, it = C.c_int(0), C.c_int(-1)
    ptr = lambda a: None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)
    st = fn(C.c_int(K), C.c_int(V), C.c_int(q["E"]), ct(q["al"]), C.byref(nrv) if rV else None,
            ptr(cv) if Cv else None, ptr(rp) if rP else None, ptr(Q), ptr(Eu), ptr(Ev), ptr(La),
            ct(q["CP_difTol"]), C.c_int(q["CP_itMax"]), C.byref(it) if CP_it else None,
            ct(q["rho"]), ct(q["condMin"]), ct(q["difRcd"]), ct(q["PFDR_difTol"]),
            C.c_int(q["PFDR_itMax"]), ptr(t) if Time else None, ptr(o) if Obj else None,
            ptr(d) if Dif else None, C.c_int(0))
    return st, cv[:max(V, 0)], rp[:nrv.value * max(K, 1)].copy(), it.value if CP_it else None


def test_optional_outputs(gpu_lib):
    p = _simplex_24x18(F32, CP_itMax=3)
    st, Cv, rP, it = raw(p)
    assert st == 0 and 1 <= it <= p["CP_itMax"] and rP.size == p["K"] * (Cv.max() + 1)
    for off in ({"Obj": False}, {"Dif": False}, {"Time": False}, {"CP_it": False},
                {"Obj": False, "Dif": False, "Time": False, "CP_it": False}):
        st, Cv2, rP2, it2 = raw(p, **off)
        assert st == 0, off
        assert same_bytes(Cv2, Cv) and same_bytes(rP2, rP), off
        if off.get("CP_it", True):
            assert it2 == it
    # Dif == NULL and CP_difTol == 0: nothing is tracked, the run goes to CP_itMax
    st, Cv0, rP0, it0 = raw(p, Dif=False, CP_difTol=0.0)
    assert st == 0 and it0 == 3
    st, Cv1, rP1, it1 = raw(p, CP_difTol=0.0)
    assert st == 0 and it1 == 3 and same_bytes(Cv0, Cv1) and same_bytes(rP0, rP1)


def test_argument_errors(gpu_lib):
    p = _simplex_24x18(F32, CP_itMax=2)
    bad = [
        ("K < 2", dict(K=1)),
        ("K < 2", dict(K=0)),
        ("V <= 0", dict(V=0)),
        ("V <= 0", dict(V=-3)),
        ("E < 0", dict(E=-1)),
        ("CP_itMax < 0", dict(CP_itMax=-1)),
        ("al < 0", dict(al=-0.1)),
        ("al > 1", dict(al=1.5)),
        ("al NaN", dict(al=float("nan"))),
        ("no Q", dict(Y=None)),
        ("no rV", dict(rV=False)),
        ("no Cv", dict(Cv=False)),
        ("no rP", dict(rP=False)),
        ("E > 0 without Eu", dict(Eu=None)),
        ("E > 0 without Ev", dict(Ev=None)),
        ("E > 0 without La_d1", dict(La_d1=None)),
    ]
    for what, over in bad:
        st, Cv, rP, it = raw(p, **over)
        msg = pfdr.load().pfdr_last_error().decode()
        assert st == 1, (what, st)  # PFDR_ERR_ARG
        assert msg.startswith("pfdr_cp_loss_d1_simplex_f32: "), (what, msg)
        assert (Cv == -1).all() and it in (-1, None), what  # nothing was written
    # the library is still usable
    st, Cv, rP, it = raw(p)
    assert st == 0 and it >= 1 and rP.size == p["K"] * (Cv.max() + 1)


# ------------------------------------- f. Python front-end and determinism --
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_python_front_end(gpu_lib, dt):
    p = _simplex_24x18(dt, CP_itMax=3)
    K, V = p["K"], p["V"]
    Q = p["Y"].reshape(V, K).T  # K-by-V
    args = (Q, p["al"], p["Eu"].astype(np.uint32), p["Ev"].astype(np.uint32), p["La_d1"],
            p["CP_difTol"], p["CP_itMax"], p["rho"], p["condMin"], p["difRcd"], p["PFDR_difTol"],
            p["PFDR_itMax"])
    Cv, rP, it, Time, Obj, Dif = pfdr.CP_PFDR_graph_loss_d1_simplex(*args)
    assert Time is None and Obj is None and Dif is None
    assert Cv.dtype == np.int32 and Cv.shape == (V,)
    rV = int(Cv.max()) + 1
    assert rP.dtype == np.dtype(dt) and rP.shape == (K, rV) and 1 <= it <= p["CP_itMax"]
    X = rP[:, Cv]
    assert X.shape == (K, V)
    assert np.all(X >= -1e-6) and np.all(np.abs(X.sum(0) - 1) <= 1e-6)
    Cv2, rP2, it2, Time, Obj, Dif = pfdr.CP_PFDR_graph_loss_d1_simplex(
        *args, time=True, obj=True, dif=True)
    assert same_bytes(Cv, Cv2) and same_bytes(rP, rP2) and it == it2
    assert Time.shape == (p["CP_itMax"] + 1,) and Time.dtype == F64
    assert Obj.shape == (p["CP_itMax"] + 1,) and Obj.dtype == np.dtype(dt)
    assert Dif.shape == (p["CP_itMax"],) and Dif.dtype == np.dtype(dt)
    assert np.all(np.diff(Time[:it + 1]) >= 0)
    # the raw entry on the same problem: the same bytes, vertex-major
    Cv3, rP3, it3 = entry(p)[:3]
    assert same_bytes(Cv, Cv3) and it == it3
    assert same_bytes(np.ascontiguousarray(rP.T).ravel(), rP3)


@pytest.mark.parametrize("kind,dt", [("kl", F32), ("labels", F64)], ids=["kl_f32", "labels_f64"])
def test_two_runs_same_bytes(gpu_lib, kind, dt):
    p, rP0, recs, runs = path_case(kind, dt)
    again = entry(p)
    for a, b in zip(runs[-1][:5], again[:5]):
        assert same_bytes(a, b) if isinstance(a, np.ndarray) else a == b
