"""The whole cut pursuit on the GPU (pfdr_cp_quadratic_d1_l1, Python
``CP_quadratic_l1``): invariants of the result, the functional against the
reference's own cut pursuit where its driver is built (oracle/_ref/cp_l1_ref,
as tests/test_dropin_cp.py runs it), and the front end's conventions.
"""
import os
import subprocess

import numpy as np
import pytest

pytest.register_assert_rewrite("cp_entry")  # its asserts report their values

import cp_problems as P
from cp_entry import constant, functional
from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

REF = os.path.join(os.path.dirname(__file__), "..", "oracle", "_ref")
REL = 1e-5

# (id, kind: l1 with positivity / l1 / differentiable single cut, A, nx, ny, dtype)
CASES = [
    ("l1pos_identity_48x40_f32", "l1pos", "identity", 48, 40, np.float32),
    ("l1pos_diag_96x80_f32", "l1pos", "diag", 96, 80, np.float32),
    ("l1_diag_48x40_f64", "l1", "diag", 48, 40, np.float64),
    ("diff_identity_96x80_f32", "diff", "identity", 96, 80, np.float32),
    ("diff_diag_48x40_f64", "diff", "diag", 48, 40, np.float64),
    ("l1_direct_20x15_f32", "l1", "direct", 20, 15, np.float32),   # V = 300, N = 200
    ("l1_direct_20x15_f64", "l1", "direct", 20, 15, np.float64),
]


def make(kind, mode, nx, ny, dt):
    over = {"N": 200} if mode == "direct" else {}
    p = P.problem("l1", mode, dt, nx, ny, **over)
    if kind == "diff":
        p["La_l1"] = None
    p["positivity"] = 1 if kind == "l1pos" else 0
    return p


def run_gpu(p, CP_itMax=None):
    return pfdr.Lib().cp_quadratic_d1_l1(
        p["V"], p["N"], p["Y"], p["A"], p["Eu"], p["Ev"], p["La_d1"], p["La_l1"],
        positivity=p["positivity"], CP_difTol=p["CP_difTol"],
        CP_itMax=p["CP_itMax"] if CP_itMax is None else CP_itMax, rho=p["rho"],
        condMin=p["condMin"], difRcd=p["difRcd"], difTol=p["PFDR_difTol"], itMax=p["PFDR_itMax"])


def components_connected(p, Cv, rV):
    parent = np.arange(p["V"])

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for u, v in zip(p["Eu"], p["Ev"]):
        if Cv[u] == Cv[v]:
            parent[find(u)] = find(v)
    roots = {find(v) for v in range(p["V"])}
    return len(roots) == rV


_results = {}


def result(cid):
    if cid not in _results:
        kind, mode, nx, ny, dt = next(c[1:] for c in CASES if c[0] == cid)
        p = make(kind, mode, nx, ny, dt)
        _results[cid] = (p, run_gpu(p))
    return _results[cid]


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_invariants(gpu_lib, cid):
    p, (Cv, rX, it, Obj, Dif, Time) = result(cid)
    rV = rX.size
    assert Cv.shape == (p["V"],) and Cv.min() == 0 and Cv.max() == rV - 1
    assert np.unique(Cv).size == rV and rV > 1
    assert components_connected(p, Cv, rV)
    assert np.all(np.isfinite(rX))
    if p["positivity"]:
        assert np.all(rX >= 0)
    assert 1 <= it <= p["CP_itMax"]
    assert Dif[it - 1] < p["CP_difTol"] ** 2 or it == p["CP_itMax"]
    o = Obj[: it + 1].astype(np.float64) + constant(p)  # the functional itself
    x = rX[Cv]
    print(cid, "rV", rV, "CP_it", it, "Obj", o, "Dif", Dif[:it], "Time", Time[: it + 1])
    assert np.all(o >= 0)
    assert np.all(o[2:] <= o[1:-1] * (1 + REL)), o
    assert np.all(np.diff(Time[: it + 1]) >= 0)
    F = functional(p, x) + constant(p)
    print(cid, "Obj[CP_it]", o[it], "F", F, "rel", abs(o[it] - F) / F)
    assert abs(o[it] - F) <= REL * F


def _ref_run(p, tmp_path, tag):
    drv = P.driver("l1", "ref", REF)
    inp, out = str(tmp_path / (tag + "_in.bin")), str(tmp_path / (tag + "_out.bin"))
    P.write(inp, p)
    r = subprocess.run([drv, inp, out], timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rV, it, Cv, rX = P.read(out, p)
    return rX[Cv]


@pytest.mark.skipif(not os.path.exists(P.driver("l1", "ref", REF)),
                    reason="reference CP driver not built here")
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_against_reference_cut_pursuit(gpu_lib, tmp_path, cid):
    """|F(GPU) - F(ref f64)| <= F(ref f64) max(1e-5, 4 gap_ref), gap_ref the
    relative difference in F between the reference's own f32 and f64 runs: the
    GPU run differs from the reference in the cut's tie-breaking and in PFDR's
    f32 path, each of the size gap_ref measures.  Two-sided: an F far below the
    reference's f64 optimum means another problem was solved."""
    p, (Cv, rX, it, Obj, Dif, Time) = result(cid)
    kind, mode, nx, ny, dt = next(c[1:] for c in CASES if c[0] == cid)
    x64 = _ref_run(make(kind, mode, nx, ny, np.float64), tmp_path, "f64")
    x32 = _ref_run(make(kind, mode, nx, ny, np.float32), tmp_path, "f32")
    p64 = make(kind, mode, nx, ny, np.float64)  # one yardstick: the f64 problem
    F64, F32, Fg = (functional(p64, x) + constant(p64) for x in (x64, x32, rX[Cv]))
    gap_ref = abs(F32 - F64) / F64
    gap = (Fg - F64) / F64
    print(cid, "F ref f64 %.9g f32 %.9g GPU %.9g gap_ref %.3e gap %.3e" % (F64, F32, Fg,
                                                                       gap_ref, gap))
    assert abs(Fg - F64) <= F64 * max(REL, 4 * gap_ref)


def test_front_end_conventions(gpu_lib):
    p = make("l1", "diag", 48, 40, np.float32)
    V, dt = p["V"], np.float32
    lib = pfdr.Lib()
    kw = dict(CP_difTol=1e-3, CP_itMax=4, rho=1.0, condMin=1e-3, difRcd=0.0, difTol=1e-4,
              itMax=10000)
    obs = (p["Y"] / p["A"]).astype(dt)
    a = np.sqrt(p["A"]).astype(dt)
    # vector A: the binding premultiplies (obs * A, A * A)
    Cv, rX = pfdr.CP_quadratic_l1(obs, p["Eu"].astype(np.uint32), p["Ev"].astype(np.uint32),
                                  0.3, a, 0.02, CP_itMax=4)
    want = lib.cp_quadratic_d1_l1(V, 0, (obs * a).astype(dt), (a * a).astype(dt), p["Eu"],
                                  p["Ev"], np.full(p["E"], 0.3, dt), np.full(V, 0.02, dt), **kw)
    assert Cv.dtype == np.uint32 and np.array_equal(Cv, want[0]) and np.array_equal(rX, want[1])
    # scalar A: identity
    Cv, rX = pfdr.CP_quadratic_l1(obs, p["Eu"], p["Ev"], p["La_d1"], 1.0, p["La_l1"], CP_itMax=4)
    want = lib.cp_quadratic_d1_l1(V, 0, obs, None, p["Eu"], p["Ev"], p["La_d1"], p["La_l1"], **kw)
    assert np.array_equal(Cv, want[0]) and np.array_equal(rX, want[1])


def test_no_iteration_returns_the_initial_solution(gpu_lib):
    p = make("l1", "diag", 48, 40, np.float64)
    Cv, rX, it, Obj, Dif, Time = run_gpu(p, CP_itMax=0)
    assert it == 0 and rX.size == 1 and not Cv.any()
    # initialize(): prox of l1 over the least-squares constant (:94-140)
    rY, rAA, la = p["Y"].sum(), p["A"].sum(), p["La_l1"].sum()
    x0 = (rY - la) / rAA if rY > la else (rY + la) / rAA if rY < -la else 0.0
    assert abs(rX[0] - x0) <= 1e-12 * abs(x0)
    F0 = functional(p, np.full(p["V"], rX[0])) + constant(p)
    assert abs(Obj[0] + constant(p) - F0) <= 1e-9 * F0
