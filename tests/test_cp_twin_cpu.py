"""The step-composed twin of the cut-pursuit driver (tests/cp_twin.py) against
the reference's recorded iterations, on the CPU.

* Always: over the oracle backend with the recorded segments as the maxflow,
  every recorded iteration of the ten l1-driver fixtures, started from its
  recorded input state, must give the recorded Cv, rX, activity and reduced
  problem bit for bit.  PFDR is actually run (the C restatement, pinned to the
  reference elsewhere), so this pins the twin's PFDR call: the reduced N, Y,
  A, L, Ltype = DIAG, start from zero, and the recorder's parameters.
* Where oracle/_ref is built: the reference's continuous driver with
  CP_itMax = k returns exactly the k-th recorded state (the fixtures were
  recorded one iteration per call through a warm restart; for N = 0 the
  restart carries everything the next iteration reads, so the chain is the
  one-call run), and the twin over the reference's BK maxflow reproduces the
  chain end to end from initialize().
* The whole-run fixtures tests/golden/cp_run/ are complete and belong to the
  inputs cp_problems.problem() generates today.
"""
import os
import subprocess

import numpy as np
import pytest

import cp_problems as P
import cp_run_cases as RC
import cp_twin as T
from cp_fixtures import NAMES, iteration_state, load_case
from oracle import CPStepRef

REF = os.path.join(os.path.dirname(__file__), "..", "oracle", "_ref")
# the recorder's PFDR parameters: oracle.CPStepRef.step's defaults
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=1000)
HAVE_REF = os.path.exists(P.driver("l1", "ref", REF)) and CPStepRef.available()


def twin_for(o, maxflow, c):
    V = c["Y"].size
    b = T.OracleBackend(o, maxflow, V, c["Eu"], c["Ev"], c["La_d1"], c["La_l1"])
    return T.Twin(b, V, 0, c["Y"], c["A"], positivity=c["positivity"], CP_difTol=c["CP_difTol"],
                  La_l1=c["La_l1"], **STEP)


def case_problem(c, CP_itMax):
    """the fixture's inputs as a cp_problems dict for the reference's driver"""
    dt = c["Y"].dtype.type
    return dict(kind="l1", V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=dt, CP_itMax=CP_itMax,
                PFDR_itMax=STEP["itMax"], positivity=c["positivity"], CP_difTol=c["CP_difTol"],
                PFDR_difTol=STEP["difTol"], rho=STEP["rho"], condMin=STEP["condMin"],
                difRcd=STEP["difRcd"], lo=-np.inf, hi=np.inf, al=0.0, Y=c["Y"], A=c["A"],
                Eu=c["Eu"], Ev=c["Ev"], La_d1=c["La_d1"], La_l1=c["La_l1"])


def assert_record(rec, d, k):
    new = iteration_state(d, k, "out")
    if rec["activated"] == 0:
        assert ("k%d_red_rEu" % k) not in d.files
    else:
        for key in ("Vc", "rVc"):
            assert np.array_equal(rec[key], new[key]), (k, key)
        red = rec["reduced"]
        for key in ("rEu", "rEv", "rLa_d1", "rY", "rAA"):
            assert np.array_equal(red[key], d["k%d_red_%s" % (k, key)]), (k, key)
        if red["rLa_l1"] is not None:
            assert np.array_equal(red["rLa_l1"], d["k%d_red_rLa_l1" % k]), k
    assert np.array_equal(rec["Cv"], new["Cv"]), k
    assert rec["rX"].dtype == new["rX"].dtype and np.array_equal(rec["rX"], new["rX"]), k
    assert np.array_equal(rec["active"], new["active"]), k


def test_ten_fixtures():
    assert len(NAMES) == 10, NAMES


@pytest.mark.parametrize("name", NAMES)
def test_twin_replays_recorded_iterations(oracle_port, name):
    c, d = load_case(name)
    kinds = set()
    for k in range(int(d["meta_steps"])):
        segs = ([d["k%d_seg_first" % k]] if ("k%d_seg_first" % k) in d.files else [])
        segs.append(d["k%d_seg_last" % k])
        it = iter(segs)
        t = twin_for(oracle_port, lambda tr, rc: next(it), c)
        t.restart(iteration_state(d, k, "in"))
        rec = t.iterate()
        assert len(rec["segments"]) == len(segs)
        assert_record(rec, d, k)
        kinds.add(rec["activated"] > 0)
        if rec["activated"]:
            assert rec["preAt"] is True and 0 < rec["pfdr_it"] <= STEP["itMax"]
    assert True in kinds


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
def test_twin_initialize_is_the_reference_s(oracle_port):
    """against the reference's own initialize() as built here (no OpenMP: sums
    in order).  The fixtures' k0_in_rX is NOT that value in 9 of the 10 files:
    it differs in the last bits, as a sum split over threads does, so it was
    recorded from a build whose initialize() reduced in parallel.  Nothing
    after the first cut reads it -- every reduced solve starts from zero -- and
    the first cut is the same from either value (the continuous runs below
    start from the sequential one and land on the recorded k0_out state)."""
    ref = CPStepRef()
    differs = 0
    for name in NAMES:
        c, d = load_case(name)
        rX0 = twin_for(oracle_port, None, c).initialize()
        want = ref.init(c["Y"], c["A"], c["Eu"], c["Ev"], c["La_d1"], c["La_l1"], c["positivity"])
        assert rX0.dtype == want.dtype and np.array_equal(rX0, want), name
        rec = d["k0_in_rX"]
        # two orders of the same V-term sums: each within gamma_V of the exact sum
        V, u = c["Y"].size, float(np.finfo(rec.dtype).eps) / 2
        g = V * u / (1 - V * u)
        num = np.abs(c["Y"]).sum(dtype=np.float64)
        if c["La_l1"] is not None:
            num += np.abs(c["La_l1"]).sum(dtype=np.float64)
        den = float(V) if c["A"] is None else c["A"].sum(dtype=np.float64)
        bound = 2 * g * num / den + 2 * (g + 2 * u) * abs(float(want[0]))
        assert abs(float(rec[0]) - float(want[0])) <= bound, name
        differs += not np.array_equal(rec, want)
    print("k0_in_rX differs from the sequential initialize() in %d of %d" % (differs, len(NAMES)))


def _continuous(c, k, tmp_path):
    drv = P.driver("l1", "ref", REF)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    p = case_problem(c, k)
    P.write(inp, p)
    r = subprocess.run([drv, inp, out], timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return P.read(out, p)


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", NAMES)
def test_continuous_reference_run_is_the_recorded_chain(oracle_port, tmp_path, name):
    """The premise of the exact GPU test: cp_l1_ref with CP_itMax = k returns
    k{it-1}_out_Cv / _out_rX, it the returned CP_it (k, or fewer once the
    iterate evolution falls below CP_difTol^2, which the warm-restart chain
    never applies).  It holds for all ten fixtures, f32 and f64."""
    c, d = load_case(name)
    steps = int(d["meta_steps"])
    last = 0
    for k in range(1, steps + 1):
        rV, it, Cv, rX = _continuous(c, k, tmp_path)
        assert 1 <= it <= k and it >= last
        assert it == k or it == last, "stopped early once, stays stopped"
        last = it
        assert np.array_equal(Cv, d["k%d_out_Cv" % (it - 1)]), (k, it)
        assert np.array_equal(rX, d["k%d_out_rX" % (it - 1)]), (k, it)
        assert rV == rX.size


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", NAMES)
def test_twin_reproduces_the_chain_end_to_end(oracle_port, tmp_path, name):
    """from initialize(), with the reference's own BK maxflow: every iteration
    the twin runs is the recorded one, and it stops where the reference's
    continuous driver stops"""
    c, d = load_case(name)
    ref = CPStepRef()
    steps = int(d["meta_steps"])
    t = twin_for(oracle_port, lambda tr, rc: ref.maxflow(c["Eu"], c["Ev"], tr, rc), c)
    rX0, recs = t.run(steps)
    assert np.array_equal(rX0, ref.init(c["Y"], c["A"], c["Eu"], c["Ev"], c["La_d1"], c["La_l1"],
                                        c["positivity"]))
    for k, rec in enumerate(recs):
        assert_record(rec, d, k)
    _, it, _, _ = _continuous(c, steps, tmp_path)
    assert len(recs) == it


# ------------------------------------------------ the whole-run fixtures --
def test_cp_run_fixtures_complete():
    have = sorted(f[:-4] for f in os.listdir(RC.DIR) if f.endswith(".npz"))
    assert have == sorted(RC.NAMES)
    for name in RC.NAMES:
        path = os.path.join(RC.DIR, name + ".npz")
        assert os.path.getsize(path) < 100 * 1024, name
        assert sorted(np.load(path).files) == ["CP_it", "Cv", "hash", "rX"], name


@pytest.mark.parametrize("name", RC.NAMES)
def test_cp_run_fixture_belongs_to_todays_inputs(name):
    p = RC.by_name(name)
    g = RC.load(name)
    assert g["hash"] == RC.input_hash(p)
    assert g["Cv"].shape == (p["V"],) and g["Cv"].dtype == np.int32
    assert g["rX"].dtype == np.dtype(p["dtype"]) and g["rX"].size == g["Cv"].max() + 1
    assert 1 <= g["CP_it"] <= p["CP_itMax"]
    if name.startswith("nothing"):
        assert g["rX"].size == 1 and g["CP_it"] == 1
