"""The step-composed twin of the duplex cut-pursuit driver
(tests/cp_twin.py, flavour "duplex") against the reference's recorded iterations
(tests/golden/cp_duplex_*.npz), on the CPU.

* Always: over the oracle backend, every recorded iteration of the eight
  duplex fixtures, started from its recorded input state with the recorded
  2V segments for the cut, gives the recorded Cv, Vc, rVc, rX, activity and
  reduced problem bit for bit.  PFDR is actually run (the C restatement), so
  this pins the twin's PFDR call: positivity, the reduced Y, A, L,
  Ltype = DIAG, the start from zero, and the recorder's parameters.
* Where oracle/_ref is built: the reference's continuous driver cp_duplex_ref
  with CP_itMax = n returns exactly k{it-1}_out, it the returned CP_it, for
  n = 1..6 (the fixtures were
  recorded one iteration per call through the step harness, which guards the
  reference's read of Cv[V], :588; the command-line driver does not -- this
  shows the continuous run was not disturbed), and the twin over the
  reference's own two-layer maxflow reproduces the chain end to end from
  initialize().
* The whole-run fixtures tests/golden/cp_duplex_run/ are complete and belong to
  the inputs cp_problems.problem() generates today.
"""
import os
import subprocess

import numpy as np
import pytest

import cp_duplex_run_cases as RC
import cp_twin as T
import cp_problems as P
from cp_fixtures import DNAMES, iteration_state, load_case
from oracle import CPStepRefDuplex

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF = os.path.join(ROOT, "oracle", "_ref")
# the recorder's PFDR parameters: oracle.CPStepRefDuplex.step's defaults
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=1000)
HAVE_REF = os.path.exists(P.driver("duplex", "ref", REF)) and CPStepRefDuplex.available()


def twin_for(o, maxflow, c):
    V = c["Y"].size
    b = T.OracleBackend(o, maxflow, V, c["Eu"], c["Ev"], c["La_d1"], c["La_l1"], "duplex")
    return T.Twin(b, V, 0, c["Y"], c["A"], positivity=c["positivity"],
                  CP_difTol=c["CP_difTol"], La_l1=c["La_l1"], **STEP)


def case_problem(c, CP_itMax):
    """the fixture's inputs as a cp_problems dict for the reference's driver"""
    dt = c["Y"].dtype.type
    return dict(kind="duplex", V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=dt,
                CP_itMax=CP_itMax, PFDR_itMax=STEP["itMax"], positivity=c["positivity"],
                CP_difTol=c["CP_difTol"], PFDR_difTol=STEP["difTol"], rho=STEP["rho"],
                condMin=STEP["condMin"], difRcd=STEP["difRcd"], lo=-np.inf, hi=np.inf, al=0.0,
                Y=c["Y"], A=c["A"], Eu=c["Eu"], Ev=c["Ev"], La_d1=c["La_d1"], La_l1=c["La_l1"])


def assert_record(rec, d, k):
    new = iteration_state(d, k, "out")
    if rec["activated"] == 0:
        assert ("k%d_red_rEu" % k) not in d.files
    else:
        for key in ("Vc", "rVc"):
            assert np.array_equal(rec[key], new[key]), (k, key)
        red = rec["reduced"]
        for key in ("rEu", "rEv", "rLa_d1", "rLa_l1", "rY", "rAA"):
            assert np.array_equal(red[key], d["k%d_red_%s" % (k, key)]), (k, key)
    assert np.array_equal(rec["Cv"], new["Cv"]), k
    assert rec["rX"].dtype == new["rX"].dtype and np.array_equal(rec["rX"], new["rX"]), k
    assert np.array_equal(rec["active"], new["active"]), k


def test_eight_fixtures():
    assert len(DNAMES) == 8, DNAMES


@pytest.mark.parametrize("name", DNAMES)
def test_twin_replays_recorded_iterations(oracle_port, name):
    c, d = load_case(name)
    V = c["Y"].size
    kinds = set()
    for k in range(int(d["meta_steps"])):
        seg = d["k%d_seg_last" % k]
        assert seg.size == 2 * V
        t = twin_for(oracle_port, lambda tr, link, rc: seg, c)
        t.restart(iteration_state(d, k, "in"))
        rec = t.iterate()
        assert len(rec["segments"]) == 1 and np.array_equal(rec["segments"][0], seg)
        assert_record(rec, d, k)
        kinds.add(rec["activated"] > 0)
        if rec["activated"]:
            assert rec["preAt"] is True and 0 < rec["pfdr_it"] <= STEP["itMax"]
        # the twin's own l1 term and positivity come back after the cut block
        assert t.positivity == c["positivity"] and (t.La_l1 is None) == (c["La_l1"] is None)
    assert True in kinds


def _continuous(c, k, tmp_path):
    drv = P.driver("duplex", "ref", REF)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    p = case_problem(c, k)
    P.write(inp, p)
    r = subprocess.run([drv, inp, out], timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return P.read(out, p)


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", DNAMES)
def test_continuous_reference_run_is_the_recorded_chain(tmp_path, name):
    """The premise of the exact GPU test: cp_duplex_ref with CP_itMax = k returns
    k{it-1}_out_Cv / _out_rX, it the returned CP_it (k, or fewer once the
    iterate evolution falls below CP_difTol^2, which the step-by-step recording
    never applies)."""
    c, d = load_case(name)
    steps = int(d["meta_steps"])
    assert steps == 6
    last = 0
    for k in range(1, steps + 1):
        rV, it, Cv, rX = _continuous(c, k, tmp_path)
        assert 1 <= it <= k and it >= last
        assert it == k or it == last, "stopped early once, stays stopped"
        last = it
        assert np.array_equal(Cv, d["k%d_out_Cv" % (it - 1)]), (k, it)
        want = d["k%d_out_rX" % (it - 1)]
        assert rX.dtype == want.dtype and np.array_equal(rX, want), (k, it)
        assert rV == rX.size


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", DNAMES)
def test_twin_reproduces_the_chain_end_to_end(oracle_port, tmp_path, name):
    """from initialize(), with the reference's own BK maxflow on its two-layer
    graph: every iteration the twin runs is the recorded one, its
    one-component start is the reference's own initialize(), and it stops
    where the reference's continuous driver stops"""
    c, d = load_case(name)
    ref = CPStepRefDuplex()
    V = c["Y"].size
    steps = int(d["meta_steps"])
    t = twin_for(oracle_port,
                 lambda tr, link, rc: ref.maxflow(V, c["Eu"], c["Ev"], tr, link, rc), c)
    rX0, recs = t.run(steps)
    want = ref.init(c["Y"], c["A"], c["Eu"], c["Ev"], c["La_d1"], c["La_l1"], c["positivity"])
    assert rX0.dtype == want.dtype and np.array_equal(rX0, want)
    for k, rec in enumerate(recs):
        assert_record(rec, d, k)
    _, it, _, _ = _continuous(c, steps, tmp_path)
    assert len(recs) == it


def test_differentiable_case_is_the_l1_twin(oracle_port):
    """no l1 term, no positivity: the duplex flavour is the l1 flavour"""
    c, d = load_case(DNAMES[0])
    V = c["Y"].size
    seen = []

    def maxflow(tr, rc):
        seen.append(tr.size)
        return (tr < 0).astype(np.uint8)

    recs = []
    for flavour in ("l1", "duplex"):
        b = T.OracleBackend(oracle_port, maxflow, V, c["Eu"], c["Ev"], c["La_d1"], None, flavour)
        recs.append(T.Twin(b, V, 0, c["Y"], c["A"], CP_difTol=c["CP_difTol"], **STEP).run(2)[1])
    assert seen and all(n == V for n in seen)
    for a, b in zip(*recs):
        assert np.array_equal(a["Cv"], b["Cv"]) and a["rX"].tobytes() == b["rX"].tobytes()


# ------------------------------------------------ the whole-run fixtures --
def test_cp_duplex_run_fixtures_complete():
    have = sorted(f[:-4] for f in os.listdir(RC.DIR) if f.endswith(".npz"))
    assert have == sorted(RC.NAMES)
    assert len(RC.NAMES) == 10
    for name in RC.NAMES:
        path = os.path.join(RC.DIR, name + ".npz")
        assert os.path.getsize(path) < 100 * 1024, name
        assert sorted(np.load(path).files) == ["CP_it", "Cv", "hash", "rX"], name


@pytest.mark.parametrize("name", RC.NAMES)
def test_cp_duplex_run_fixture_belongs_to_todays_inputs(name):
    p = RC.by_name(name)
    g = RC.load(name)
    assert p["kind"] == "duplex" and p["La_l1"] is not None
    assert g["hash"] == RC.input_hash(p)
    assert g["Cv"].shape == (p["V"],) and g["Cv"].dtype == np.int32
    assert g["rX"].dtype == np.dtype(p["dtype"]) and g["rX"].size == g["Cv"].max() + 1
    assert 0 < g["CP_it"] <= p["CP_itMax"]
    if name.startswith("nothing"):
        assert g["rX"].size == 1
    else:
        assert g["rX"].size > 1
    if p["positivity"]:
        assert np.all(g["rX"] >= 0) and np.any(g["rX"] == 0)


@pytest.mark.parametrize("kind", RC.KINDS)
def test_reference_f32_and_f64_runs_agree(kind):
    """the reference's own two precisions: the same partition and iteration count"""
    a, b = RC.load(kind + "_f32"), RC.load(kind + "_f64")
    assert a["CP_it"] == b["CP_it"] and np.array_equal(a["Cv"], b["Cv"])
