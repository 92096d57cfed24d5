"""Two paths of the sessions' shared iteration loop (csrc/pfdr_loop.hpp) that
no other test reaches.

1. Prepared tail graphs on a NON-speculative session.  The other prepare()
   tests run speculative sessions, which launch directly (prepare returns at
   once).  Here difRcd > 0 rules speculation out, the one-workgroup path is
   switched off while the session is created, and the run is cut into pieces
   (7, 33, 1, 64, 600) with prepare(n) before each run(n): whole chunks and
   prepared tails replay hipGraphs, and every reconditioning drops the graphs,
   which are then captured again.  it, every Dif and the iterate equal the
   single-threaded restatement's, byte for byte.  The restatement's own it and
   Dif show that each case reconditions and stops before itMax (checked on the
   CPU when the cases were chosen: the quadratic ones recondition after
   iterations 5, 14 and 87 and stop at 435, the simplex after 1, 47 and 156
   and stops at 306), so the reconditionings fall into different pieces.

2. The verbose output of a session: the last progress report carries the
   result's iteration count, every "Reconditioning... " is closed by "done."
   on its line, and in the quadratic sessions a progress report (its
   "iteration" line, then its "iterate evolution" line: these sessions track
   the evolution) stands immediately before each of them.  The simplex
   session reports after a reconditioning, not before.  A label-tracking
   simplex run (difTol = 1) reports "label evolution"; it cannot recondition
   (a count of changed labels below difRcd is zero, which stops the run), so
   it is a run of its own beside the three cases.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 48
DIF_RCD = 1e-2
IT_MAX = 600
PIECES = (7, 33, 1, 64, 600)
CASES = ["l1-f32", "l1-f64", "simplex-f32"]


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _problem(case):
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import grid_graph, simplex_observation
    V = N * N
    if case == "simplex-f32":
        Eu, Ev = grid_graph((N, N), 8)
        Q = simplex_observation(V, 3, 4, (np.arange(V) % N) * 3 // N, np.float32)
        return dict(K=3, Eu=Eu.astype(np.int32), Ev=Ev.astype(np.int32), Q=Q,
                    La=np.full(Eu.size, 0.05, np.float32))
    dt = np.float32 if case == "l1-f32" else np.float64
    Eu, Ev = grid_graph((N, N), 4)
    return dict(K=0, Eu=Eu.astype(np.int32), Ev=Ev.astype(np.int32),
                Y=pfdr.gen_piecewise(N, V, 3, dt, 0.2), La=np.full(Eu.size, 0.1, dt),
                L1=np.full(V, 0.01, dt))


def _session(case, difTol=1e-5, verbose=0):
    from cp_pfdr_graph_d1_amd import pfdr
    p = _problem(case)
    V = N * N
    common = dict(difRcd=DIF_RCD, difTol=difTol, itMax=IT_MAX, record_dif=True,
                  evolution=pfdr.EVOLUTION_SEQUENTIAL, verbose=verbose)
    if p["K"]:
        with _env(PFDR_SX_TINY="0"):
            return pfdr.Session(pfdr.PFDR_KIND_SIMPLEX, np.float32, V, p["Eu"].size, p["Eu"],
                                p["Ev"], p["La"], p["Q"].copy(), p["Q"], K=p["K"], al=0.1, rho=1.0,
                                condMin=0.1, **common)
    dt = p["Y"].dtype
    with _env(PFDR_TINY="0"):
        return pfdr.Session(pfdr.PFDR_KIND_L1, dt, V, p["Eu"].size, p["Eu"], p["Ev"], p["La"],
                            np.zeros(V, dt), p["Y"], La_l1=p["L1"], rho=1.5, condMin=1e-3,
                            **common)


@functools.lru_cache(maxsize=None)
def _restatement(case, difTol=1e-5):
    """(X, it, Dif) of the single-threaded restatement; shared, not modified"""
    import oracle
    from cp_pfdr_graph_d1_amd import pfdr
    p = _problem(case)
    V = N * N
    o = oracle.Oracle("port")
    if p["K"]:
        X, it, _, Dif = o.loss_d1_simplex(p["Q"].copy(), p["Q"], p["K"], p["Eu"], p["Ev"], p["La"],
                                          0.1, None, 1.0, 0.1, DIF_RCD, difTol, IT_MAX, dif=True)
    else:
        dt = p["Y"].dtype
        X, it, _, Dif = o.quadratic_d1_l1(np.zeros(V, dt), p["Y"], None, 0, p["Eu"], p["Ev"],
                                          p["La"], p["L1"], 0, pfdr.SCAL, None, 1.5, 1e-3, DIF_RCD,
                                          difTol, IT_MAX, dif=True)
    return X, it, Dif


def _reconditionings(case, it, Dif):
    """the iterations after which the reference loop reconditions: Dif below
    the reconditioning threshold (squared, then x 0.01 each time, in the
    quadratic solvers; x 0.1 in the simplex) on an iteration that did not stop"""
    dt = Dif.dtype.type
    rcd, f = (dt(DIF_RCD), dt(0.1)) if case == "simplex-f32" else \
        (dt(DIF_RCD) * dt(DIF_RCD), dt(0.01))
    out = []
    for k in range(it - 1):
        if Dif[k] < rcd:
            out.append(k + 1)
            rcd = rcd * f
    return out


@pytest.mark.parametrize("case", CASES)
def test_prepared_tails_on_a_plain_session_match_restatement(gpu_lib, oracle_port, case):
    Xo, ito, Difo = _restatement(case)
    rc = _reconditionings(case, ito, Difo)
    print("%s: restatement it %d, reconditions after %s" % (case, ito, rc))
    assert len(rc) >= 1 and ito < IT_MAX, "the case must recondition and stop: pick another"
    s = _session(case)
    try:
        assert s.query("graphs") == 1
        assert s.query("speculative") == 0
        assert s.query("tiny") == 0
        for n in PIECES:
            s.prepare(n)
            s.run(n)
        X, it, _, Dif = s.result()
    finally:
        s.close()
    print("%s: it %d / %d" % (case, it, ito))
    assert it == ito
    assert np.array_equal(Dif[:it], Difo[:ito])
    assert np.array_equal(X, Xo)


def _verbose_run(case, difTol=1e-5):
    """one verbose run to the end; returns the result's it (stdout: the caller's)"""
    s = _session(case, difTol=difTol, verbose=1)
    try:
        s.run(IT_MAX)
        it = s.result()[1]
    finally:
        s.close()
    return it


@pytest.mark.parametrize("case", CASES)
def test_verbose_output_of_a_session(gpu_lib, case, capfd):
    capfd.readouterr()
    it = _verbose_run(case)
    out = capfd.readouterr().out
    print(out)
    lines = out.splitlines()
    reports = [ln for ln in lines if ln.startswith("iteration ")]
    assert reports and reports[-1] == "iteration %d (max. %d)" % (it, IT_MAX)
    rc = [i for i, ln in enumerate(lines) if "Reconditioning... " in ln]
    assert len(rc) >= 1
    for i in rc:
        assert lines[i] == "Reconditioning... done."
        if case != "simplex-f32":
            assert i >= 2 and lines[i - 2].startswith("iteration ") and \
                lines[i - 1].startswith("iterate evolution ")
    assert "iterate evolution " in out and "label evolution" not in out


def test_verbose_simplex_reports_label_evolution(gpu_lib, capfd):
    capfd.readouterr()
    it = _verbose_run("simplex-f32", difTol=1.0)
    out = capfd.readouterr().out
    print(out)
    reports = [ln for ln in out.splitlines() if ln.startswith("iteration ")]
    assert reports and reports[-1] == "iteration %d (max. %d)" % (it, IT_MAX)
    assert "label evolution " in out and "iterate evolution" not in out
