"""The bounds driver's one-call cut pursuit (pfdr_cp_quadratic_d1_bounds, the
bounds flavour of csrc/pfdr_cutpursuit.hip) pinned on every path of its loop:
the bounds flavour's cases of the checks in tests/cp_entry_checks.py, a. to h.
there, over all ten iteration fixtures and the nine recorded-run cases in both
types, and what only this flavour has: verbose changes nothing, and the A^tA
front end.
"""
import numpy as np
import pytest

# the shared bodies' asserts report their values like a test module's
pytest.register_assert_rewrite("cp_entry", "cp_entry_checks")

import cp_bounds_run_cases as RC
import cp_entry_checks as K
from cp_entry import F32, F64, _same_result, entry, same_bytes
from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

FL = "bounds"
PATH_IDS = K.PATH_IDS[FL]
_ids = K.path_ids(PATH_IDS)


@pytest.mark.parametrize("name", K.FIXTURES[FL])
def test_entry_is_the_reference_run(gpu_lib, name):
    K.entry_is_the_reference_run(FL, name)


def test_all_ten_fixtures_are_run():
    assert len(K.FIXTURES[FL]) == 10, K.FIXTURES[FL]


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_entry_is_the_twin(gpu_lib, kind, dt):
    K.entry_is_the_twin(FL, kind, dt)


@pytest.mark.parametrize("name", [n for n in RC.NAMES if RC.by_name(n)["N"] == 0])
def test_recorded_run_exact(gpu_lib, name):
    K.recorded_run_exact(FL, name)


@pytest.mark.parametrize("kind", ["direct12", "direct160", "AtA"])
@pytest.mark.parametrize("d", ["f32", "f64"])
def test_recorded_run_functional(gpu_lib, kind, d):
    K.recorded_run_functional(FL, d, kind)


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_obj_and_dif_at_every_iteration(gpu_lib, kind, dt):
    K.obj_and_dif_at_every_iteration(FL, kind, dt)


@pytest.mark.parametrize("name", ["cp_bounds_box_f32", "cp_bounds_knn_diag_f64"])
def test_obj_and_dif_on_fixtures(gpu_lib, name):
    K.obj_and_dif_on_fixtures(FL, name)


def test_optional_outputs_and_repeatability(gpu_lib):
    K.optional_outputs_and_repeatability(FL)


def test_verbose_changes_nothing(gpu_lib, capfd):
    p = RC.problem("clamp_lo", F32)
    a = entry("bounds", p)
    b = entry("bounds", p, verbose=1000)
    out = capfd.readouterr().out
    assert a[2] == b[2] and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    # the l1 entry's lines, one block per iteration and the closing one
    assert out.count("Cut pursuit iteration") == a[2] + 1, out
    assert "Cut pursuit iteration 0 (max. %d)" % p["CP_itMax"] in out
    assert "1 connected component(s), 0 reduced edge(s)" in out
    assert "relative iterate evolution" in out


def test_argument_errors(gpu_lib):
    K.argument_errors(FL)


@pytest.mark.parametrize("kind", ["direct12", "free_diag", "nothing"])
def test_stats(gpu_lib, kind):
    K.stats(FL, kind)


def test_mex_quadratic(gpu_lib):
    K.mex_quadratic(FL)


def test_mex_AtA(gpu_lib):
    p = RC.problem("AtA", F64)
    V = p["V"]
    AtA = np.asarray(p["A"]).reshape(V, V).T
    got = pfdr.CP_PFDR_graph_quadratic_d1_bounds_AtA(p["Y"], AtA, p["Eu"], p["Ev"], p["La_d1"],
                                                     (p["lo"], p["hi"]), *K.PAR, time=True,
                                                     obj=True, dif=True)
    Obj, wObj = _same_result(got, entry("bounds", p, CP_itMax=K.PAR[1]), K.PAR[1])
    assert same_bytes(Obj, wObj)


def test_mex_l22(gpu_lib):
    K.mex_l22(FL)
