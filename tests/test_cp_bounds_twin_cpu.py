"""The step-composed twin of the bounds cut-pursuit driver
(tests/cp_twin.py, flavour "bounds") against the reference's recorded iterations
(tests/golden/cp_bounds_*.npz), on the CPU.

* Always: over the oracle backend, every recorded iteration of the ten
  bounds-driver fixtures, started from its recorded input state, gives the
  recorded Cv, Vc, rVc, rX, activity and reduced problem bit for bit.  The
  maxflow is the reference's BK where oracle/_ref is built, the recorded
  segments otherwise.  PFDR is actually run (the C restatement), so this pins
  the twin's PFDR call: the box, the reduced N, Y, A, L, Ltype = DIAG, the
  start from zero, and the recorder's parameters.
* Where oracle/_ref is built: the reference's continuous driver cp_bounds_ref
  with CP_itMax = n returns exactly k{n-1}_out for n = 1..6 (the fixtures were
  recorded one iteration per call through a warm restart), and the twin over
  the reference's maxflow reproduces the chain end to end from initialize().
* The header declares the one-call entries and their stats call, and the
  library exports them.
* The whole-run fixtures tests/golden/cp_bounds_run/ are complete and belong
  to the inputs cp_problems.problem() generates today.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import cp_bounds_run_cases as RC
import cp_twin as T
import cp_problems as P
from cp_fixtures import BNAMES, iteration_state, load_case
from oracle import CPStepRef, CPStepRefBounds

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF = os.path.join(ROOT, "oracle", "_ref")
# the recorder's PFDR parameters: oracle.CPStepRefBounds.step's defaults
STEP = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-4, itMax=1000)
HAVE_REF = (os.path.exists(P.driver("bounds", "ref", REF)) and CPStepRef.available()
            and CPStepRefBounds.available())
ENTRIES = ("pfdr_cp_quadratic_d1_bounds_f32", "pfdr_cp_quadratic_d1_bounds_f64",
           "pfdr_cp_quadratic_d1_bounds_stats")


def twin_for(o, maxflow, c):
    V = c["Y"].size
    b = T.OracleBackend(o, maxflow, V, c["Eu"], c["Ev"], c["La_d1"], None, "bounds", c["lo"],
                        c["hi"])
    return T.Twin(b, V, 0, c["Y"], c["A"], CP_difTol=c["CP_difTol"], **STEP)


def case_problem(c, CP_itMax):
    """the fixture's inputs as a cp_problems dict for the reference's driver"""
    dt = c["Y"].dtype.type
    return dict(kind="bounds", V=c["Y"].size, E=c["Eu"].size, N=0, K=0, dtype=dt,
                CP_itMax=CP_itMax, PFDR_itMax=STEP["itMax"], positivity=0,
                CP_difTol=c["CP_difTol"], PFDR_difTol=STEP["difTol"], rho=STEP["rho"],
                condMin=STEP["condMin"], difRcd=STEP["difRcd"], lo=c["lo"], hi=c["hi"], al=0.0,
                Y=c["Y"], A=c["A"], Eu=c["Eu"], Ev=c["Ev"], La_d1=c["La_d1"], La_l1=None)


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
        assert red["rLa_l1"] is None
    assert np.array_equal(rec["Cv"], new["Cv"]), k
    assert rec["rX"].dtype == new["rX"].dtype and np.array_equal(rec["rX"], new["rX"]), k
    assert np.array_equal(rec["active"], new["active"]), k


def recorded_segments(d, k):
    segs = [d["k%d_seg_first" % k]] if ("k%d_seg_first" % k) in d.files else []
    segs.append(d["k%d_seg_last" % k])
    return segs


def test_ten_fixtures():
    assert len(BNAMES) == 10, BNAMES


@pytest.mark.parametrize("name", BNAMES)
def test_twin_replays_recorded_iterations(oracle_port, name):
    c, d = load_case(name)
    free = c["lo"] == -np.inf and c["hi"] == np.inf
    ref = CPStepRef() if CPStepRef.available() else None
    kinds = set()
    for k in range(int(d["meta_steps"])):
        segs = recorded_segments(d, k)
        if ref is not None:  # the reference's own BK maxflow on the twin's capacities
            maxflow = lambda tr, rc: ref.maxflow(c["Eu"], c["Ev"], tr, rc)
        else:                # the recorded segments
            it = iter(segs)
            maxflow = lambda tr, rc: next(it)
        t = twin_for(oracle_port, maxflow, c)
        t.restart(iteration_state(d, k, "in"))
        rec = t.iterate()
        assert len(rec["segments"]) == (1 if free else 2)
        assert np.array_equal(rec["segments"][-1], segs[-1]), k
        if len(segs) == 2:
            assert np.array_equal(rec["segments"][0], segs[0]), k
        assert_record(rec, d, k)
        kinds.add(rec["activated"] > 0)
        if rec["activated"]:
            assert rec["preAt"] is True and 0 < rec["pfdr_it"] <= STEP["itMax"]
    assert True in kinds


def test_final_states_sit_on_their_bounds():
    """what makes the fixtures a yardstick for the +inf capacities: in the last
    recorded state some component is exactly at a bound in every file that has one"""
    at = 0
    for name in BNAMES:
        c, d = load_case(name)
        rX = d["k%d_out_rX" % (int(d["meta_steps"]) - 1)]
        real = rX.dtype.type
        assert np.all(rX >= real(c["lo"])) and np.all(rX <= real(c["hi"])), name
        n = int(np.count_nonzero((rX == real(c["lo"])) | (rX == real(c["hi"]))))
        if "free" in name:
            assert n == 0
        at += n > 0
    assert at == 8, at


def _continuous(c, k, tmp_path):
    drv = P.driver("bounds", "ref", REF)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    p = case_problem(c, k)
    P.write(inp, p)
    r = subprocess.run([drv, inp, out], timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return P.read(out, p)


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", BNAMES)
def test_continuous_reference_run_is_the_recorded_chain(tmp_path, name):
    """The premise of the exact GPU test: cp_bounds_ref with CP_itMax = n returns
    k{n-1}_out_Cv / _out_rX for n = 1..6, and no run stops early."""
    c, d = load_case(name)
    steps = int(d["meta_steps"])
    assert steps == 6
    for n in range(1, steps + 1):
        rV, it, Cv, rX = _continuous(c, n, tmp_path)
        assert it == n, (n, it)
        assert np.array_equal(Cv, d["k%d_out_Cv" % (n - 1)]), n
        want = d["k%d_out_rX" % (n - 1)]
        assert rX.dtype == want.dtype and np.array_equal(rX, want), n
        assert rV == rX.size


@pytest.mark.skipif(not HAVE_REF, reason="reference CP driver not built here")
@pytest.mark.parametrize("name", BNAMES)
def test_twin_reproduces_the_chain_end_to_end(oracle_port, name):
    """from initialize(), with the reference's own BK maxflow: every iteration
    the twin runs is the recorded one; its one-component start is the
    reference's own initialize()"""
    c, d = load_case(name)
    ref = CPStepRef()
    steps = int(d["meta_steps"])
    t = twin_for(oracle_port, lambda tr, rc: ref.maxflow(c["Eu"], c["Ev"], tr, rc), c)
    rX0, recs = t.run(steps)
    want = CPStepRefBounds().init(c["Y"], c["A"], c["Eu"], c["Ev"], c["La_d1"], c["lo"], c["hi"])
    assert rX0.dtype == want.dtype and np.array_equal(rX0, want)
    assert len(recs) == steps
    for k, rec in enumerate(recs):
        assert_record(rec, d, k)


# ------------------------------------------------------ the public surface --
def test_header_declares_and_library_exports_the_entries():
    from cp_pfdr_graph_d1_amd import pfdr
    txt = open(os.path.join(ROOT, "include", "pfdr_mi355x.h")).read()
    declared = set(re.findall(r"^int (pfdr_[a-z0-9_]+)\s*\(", txt, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", pfdr.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ENTRIES:
        assert name in declared, name
        assert name in exported, name
        assert name in pfdr.EXPORTED, name
    assert pfdr.load().pfdr_abi_version() == 4
    for name in ("cp_quadratic_d1_bounds", "cp_quadratic_d1_bounds_stats"):
        assert callable(getattr(pfdr.Lib, name))
    for name in ("CP_PFDR_graph_quadratic_d1_bounds", "CP_PFDR_graph_quadratic_d1_bounds_AtA",
                 "CP_PFDR_graph_l22_d1_bounds"):
        assert callable(getattr(pfdr, name))


# ------------------------------------------------ the whole-run fixtures --
def test_cp_bounds_run_fixtures_complete():
    have = sorted(f[:-4] for f in os.listdir(RC.DIR) if f.endswith(".npz"))
    assert have == sorted(RC.NAMES)
    assert len(RC.NAMES) == 18
    for name in RC.NAMES:
        path = os.path.join(RC.DIR, name + ".npz")
        assert os.path.getsize(path) < 100 * 1024, name
        assert sorted(np.load(path).files) == ["CP_it", "Cv", "hash", "rX"], name


@pytest.mark.parametrize("name", RC.NAMES)
def test_cp_bounds_run_fixture_belongs_to_todays_inputs(name):
    p = RC.by_name(name)
    g = RC.load(name)
    assert g["hash"] == RC.input_hash(p)
    assert g["Cv"].shape == (p["V"],) and g["Cv"].dtype == np.int32
    assert g["rX"].dtype == np.dtype(p["dtype"]) and g["rX"].size == g["Cv"].max() + 1
    rV, it, lo, hi = RC.EXPECT[name.rsplit("_", 1)[0]]
    assert (g["rX"].size, g["CP_it"]) == (rV, it)
    assert RC.at_bounds(p, g["rX"]) == (lo, hi)
    real = np.dtype(p["dtype"]).type
    assert np.all(g["rX"] >= real(p["lo"])) and np.all(g["rX"] <= real(p["hi"]))


@pytest.mark.parametrize("kind", RC.KINDS)
def test_reference_f32_and_f64_runs_agree(kind):
    """the reference's own two precisions: the same partition and iteration count"""
    a, b = RC.load(kind + "_f32"), RC.load(kind + "_f64")
    assert a["CP_it"] == b["CP_it"] and np.array_equal(a["Cv"], b["Cv"])
