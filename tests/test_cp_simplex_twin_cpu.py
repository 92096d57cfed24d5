"""The step-composed twin of the simplex cut-pursuit driver
(tests/cp_simplex_twin.py) against the reference's recorded iterations
(tests/golden/cp_simplex_*.npz), on the CPU.

* Over the oracle backend, every recorded iteration of the ten simplex
  fixtures, started from its recorded input state, must give the recorded Cv,
  rP, activity, reduced problem and warm start bit for bit.  PFDR is actually
  run (the C restatement), so this pins the twin's PFDR call: warm start at
  the observations' rP, La_f = rLa_f (none for al == 0), the recorder's
  parameters.  Maxflow: the recorded segments for the K = 3 files; the
  reference's BK for K = 4 and 5 (their middle expansions are recorded too,
  but BK on the twin's own capacities also pins those), where
  oracle/_ref/libcp_step_simplex_ref.so is built.
* Where oracle/_ref/cp_simplex_ref is built: the reference's continuous driver
  with CP_itMax = n returns exactly the recorded state of its last iteration
  (the premise of the exact GPU test), with CP_difTol the smallest positive
  normal: positive, so eps stays the machine epsilon as recorded, and the run
  stops early only on an evolution of exactly zero.
* The whole-run fixtures tests/golden/cp_simplex_run/ are complete and belong
  to the inputs cp_problems.problem() generates today.
"""
import os
import subprocess

import numpy as np
import pytest

import cp_problems as P
import cp_simplex_run_cases as SR
import cp_simplex_twin as ST
from cp_fixtures import SNAMES, expansion_segments, iteration_state, load_case
from oracle import CPStepRefSimplex

REF = os.path.join(os.path.dirname(__file__), "..", "oracle", "_ref")
# the recorder's PFDR parameters: oracle.CPStepRefSimplex.step's defaults
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-3, itMax=1000)
HAVE_DRIVER = os.path.exists(P.driver("simplex", "ref", REF))


def twin_for(o, maxflow, c, CP_difTol=None):
    b = ST.OracleBackend(o, maxflow, c["K"], c["al"], c["Q"], c["Eu"], c["Ev"], c["La_d1"])
    return ST.Twin(b, c["K"], c["al"], c["Q"],
                   CP_difTol=c["CP_difTol"] if CP_difTol is None else CP_difTol, **STEP)


def case_problem(c, CP_itMax, CP_difTol=None):
    """the fixture's inputs as a cp_problems dict for the reference's driver"""
    dt = c["Q"].dtype.type
    return dict(kind="simplex", V=c["Q"].size // c["K"], E=c["Eu"].size, N=0, K=c["K"], dtype=dt,
                CP_itMax=CP_itMax, PFDR_itMax=STEP["itMax"], positivity=0,
                CP_difTol=float(np.finfo(dt).tiny) if CP_difTol is None else CP_difTol,
                PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
                difRcd=STEP["difRcd"], lo=-np.inf, hi=np.inf, al=c["al"], Y=c["Q"], A=None,
                Eu=c["Eu"], Ev=c["Ev"], La_d1=c["La_d1"], La_l1=None)


def assert_record(rec, d, k):
    new = iteration_state(d, k, "out")
    if rec["activated"] == 0:
        assert ("k%d_red_rEu" % k) not in d.files
    else:
        for key in ("Vc", "rVc"):
            assert np.array_equal(rec[key], new[key]), (k, key)
        red = rec["reduced"]
        for key in ("rEu", "rEv", "rLa_d1", "rQ", "rP0"):
            want = d["k%d_red_%s" % (k, key)]
            assert red[key].dtype == want.dtype and np.array_equal(red[key], want), (k, key)
        if red["rLa_f"] is not None:
            assert np.array_equal(red["rLa_f"], d["k%d_red_rLa_f" % k]), k
        else:
            assert ("k%d_red_rLa_f" % k) not in d.files
    assert np.array_equal(rec["Cv"], new["Cv"]), k
    assert rec["rP"].dtype == new["rP"].dtype and np.array_equal(rec["rP"], new["rP"]), k
    assert np.array_equal(rec["active"], new["active"]), k


def test_ten_fixtures():
    assert len(SNAMES) == 10, SNAMES


@pytest.mark.parametrize("name", SNAMES)
def test_twin_replays_recorded_iterations(oracle_port, name):
    c, d = load_case(name)
    K = c["K"]
    if K == 3:
        flow = None  # the recorded segments
    elif CPStepRefSimplex.available():
        ref = CPStepRefSimplex()
        flow = lambda tr, rc: ref.maxflow(c["Eu"], c["Ev"], tr, rc)
    else:
        pytest.skip("K > 3 needs the reference's maxflow, not built here")
    kinds = set()
    for k in range(int(d["meta_steps"])):
        segs = expansion_segments(d, K, k)
        it = iter(segs)
        t = twin_for(oracle_port, flow or (lambda tr, rc: next(it)), c)
        t.restart(iteration_state(d, k, "in"))
        rec = t.iterate()
        assert len(rec["segments"]) == K - 1
        for n, (a, b) in enumerate(zip(rec["segments"], segs), 1):
            assert np.array_equal(a, b), (k, n)
        assert_record(rec, d, k)
        kinds.add(rec["activated"] > 0)
        if rec["activated"]:
            assert 0 < rec["pfdr_it"] <= STEP["itMax"]
    assert True in kinds


@pytest.mark.parametrize("name", SNAMES)
def test_twin_initialize_is_the_recorded_start(oracle_port, name):
    c, d = load_case(name)
    rP0 = twin_for(oracle_port, None, c).initialize()
    want = d["k0_in_rP"]
    assert rP0.dtype == want.dtype and np.array_equal(rP0, want)


def _continuous(c, k, tmp_path):
    drv = P.driver("simplex", "ref", REF)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    p = case_problem(c, k)
    P.write(inp, p)
    r = subprocess.run([drv, inp, out], timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return P.read(out, p)


@pytest.mark.skipif(not HAVE_DRIVER, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", SNAMES)
def test_continuous_reference_run_is_the_recorded_chain(tmp_path, name):
    """cp_simplex_ref with CP_itMax = n returns k{it-1}_out_Cv / _out_rP, it
    the returned CP_it: n, or fewer once an iteration left the iterate exactly
    where it was (evolution 0 < CP_difTol), after which the run stays stopped."""
    c, d = load_case(name)
    steps = int(d["meta_steps"])
    last = 0
    for k in range(1, steps + 1):
        rV, it, Cv, rP = _continuous(c, k, tmp_path)
        assert 1 <= it <= k and it >= last
        assert it == k or it == last, "stopped early once, stays stopped"
        last = it
        assert np.array_equal(Cv, d["k%d_out_Cv" % (it - 1)]), (k, it)
        want = d["k%d_out_rP" % (it - 1)]
        assert rP.dtype == want.dtype and np.array_equal(rP, want), (k, it)
        assert rV * c["K"] == rP.size
        if it < k:  # the iteration it stopped after changed nothing
            prev = d["k%d_in_rP" % (it - 1)]
            assert np.array_equal(d["k%d_in_Cv" % (it - 1)], Cv) and np.array_equal(prev, rP)


@pytest.mark.skipif(not (HAVE_DRIVER and CPStepRefSimplex.available()),
                    reason="reference CP driver not built here")
@pytest.mark.parametrize("name", SNAMES)
def test_twin_reproduces_the_chain_end_to_end(oracle_port, tmp_path, name):
    """from initialize(), with the reference's own BK maxflow: every iteration
    the twin runs is the recorded one, and it stops where the reference's
    continuous driver stops"""
    c, d = load_case(name)
    ref = CPStepRefSimplex()
    steps = int(d["meta_steps"])
    tiny = float(np.finfo(c["Q"].dtype).tiny)
    t = twin_for(oracle_port, lambda tr, rc: ref.maxflow(c["Eu"], c["Ev"], tr, rc), c,
                 CP_difTol=tiny)
    assert t.eps == float(np.finfo(c["Q"].dtype).eps)
    rP0, recs = t.run(steps)
    for k, rec in enumerate(recs):
        assert_record(rec, d, k)
    _, it, _, _ = _continuous(c, steps, tmp_path)
    assert len(recs) == it


# ------------------------------------------------ the whole-run fixtures --
def test_cp_simplex_run_fixtures_complete():
    have = sorted(f[:-4] for f in os.listdir(SR.DIR) if f.endswith(".npz"))
    assert have == sorted(SR.NAMES)
    for name in SR.NAMES:
        path = os.path.join(SR.DIR, name + ".npz")
        assert os.path.getsize(path) < 100 * 1024, name
        assert sorted(np.load(path).files) == ["CP_it", "Cv", "hash", "rP"], name


@pytest.mark.parametrize("name", SR.NAMES)
def test_cp_simplex_run_fixture_belongs_to_todays_inputs(name):
    p = SR.by_name(name)
    g = SR.load(name)
    assert g["hash"] == SR.input_hash(p)
    assert g["Cv"].shape == (p["V"],) and g["Cv"].dtype == np.int32
    assert g["rP"].dtype == np.dtype(p["dtype"])
    assert g["rP"].size == (g["Cv"].max() + 1) * p["K"]
    assert 1 <= g["CP_it"] <= p["CP_itMax"]
