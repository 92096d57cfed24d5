"""The duplex driver's one-call cut pursuit (pfdr_cp_quadratic_d1_l1_duplex,
csrc/pfdr_cutpursuit.hip) pinned on every path of its loop: the duplex
flavour's cases of the checks in tests/cp_entry_checks.py, a. to h. there, and
what only this flavour has: the differentiable case is the bytes of
pfdr_cp_quadratic_d1_l1, verbose prints the l1 entry's lines, and the binding's
conventions.
"""
import numpy as np
import pytest

# the shared bodies' asserts report their values like a test module's
pytest.register_assert_rewrite("cp_entry", "cp_entry_checks")

import cp_duplex_run_cases as RC
import cp_entry_checks as K
import cp_problems as P
from cp_entry import F32, F64, entry, same_bytes
from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

FL = "duplex"
PATH_IDS = K.PATH_IDS[FL]
_ids = K.path_ids(PATH_IDS)


@pytest.mark.parametrize("name", K.FIXTURES[FL])
def test_entry_is_the_reference_run(gpu_lib, name):
    K.entry_is_the_reference_run(FL, name)


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_entry_is_the_twin(gpu_lib, kind, dt):
    K.entry_is_the_twin(FL, kind, dt)


@pytest.mark.parametrize("name", [n for n in RC.NAMES if n.startswith(("l1pos_diag", "nothing"))])
def test_recorded_run_exact(gpu_lib, name):
    K.recorded_run_exact(FL, name)


@pytest.mark.parametrize("kind", ["direct12", "direct160", "AtA"])
@pytest.mark.parametrize("d", ["f32", "f64"])
def test_recorded_run_functional(gpu_lib, kind, d):
    K.recorded_run_functional(FL, d, kind)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_differentiable_case_is_the_l1_entry(gpu_lib, dt):
    p = P.problem("duplex", "diag", dt, nx=48, ny=40, La_l1=None)
    assert p["La_l1"] is None and not p["positivity"]
    a, b = entry("duplex", p), entry("l1", p)
    assert a[2] == b[2] >= 1 and a[1].size > 1
    for x, y in zip(a[:5], b[:5]):  # Cv, rX, CP_it, Obj, Dif
        assert same_bytes(np.asarray(x), np.asarray(y))
    s = pfdr.Lib().cp_quadratic_d1_l1_duplex_stats()
    assert s["n_cuts"] == a[2]


@pytest.mark.parametrize("kind,dt", [("direct12", F32), ("l1pos_diag", F64)],
                         ids=["direct12_f32", "l1pos_diag_f64"])
def test_obj_and_dif_at_every_iteration(gpu_lib, kind, dt):
    K.obj_and_dif_at_every_iteration(FL, kind, dt)


def test_optional_outputs_and_repeatability(gpu_lib):
    K.optional_outputs_and_repeatability(FL)


def test_argument_errors(gpu_lib):
    K.argument_errors(FL)


def test_verbose_prints_the_l1_entrys_lines(gpu_lib, capfd):
    p = RC.problem("l1pos_diag", F32)
    a = entry("duplex", p)
    b = entry("duplex", p, verbose=1000)
    out = capfd.readouterr().out
    assert a[2] == b[2] and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    assert out.count("Cut pursuit iteration") == a[2] + 1, out
    assert "1 connected component(s), 0 reduced edge(s)" in out
    assert "DIFFERENTIABLE" not in out.upper()


@pytest.mark.parametrize("kind", ["direct12", "l1pos_diag", "nothing"])
def test_stats(gpu_lib, kind):
    K.stats(FL, kind)


def test_mex_quadratic(gpu_lib):
    K.mex_quadratic(FL)


def test_mex_l22(gpu_lib):
    K.mex_l22(FL)


def test_binding_conventions(gpu_lib):
    """CP_quadratic_l1_duplex: CP_quadratic_l1's conventions through _binding_inputs"""
    p = P.problem("duplex", "diag", F32, nx=24, ny=20, positivity=1)
    y = (np.asarray(p["Y"]) / np.asarray(p["A"])).astype(F32)
    a = np.sqrt(np.asarray(p["A"], F64)).astype(F32)
    kw = dict(positivity=1, PFDR_rho=1.5, CP_difTol=1e-4, PFDR_difTol=1e-5, CP_itMax=4,
              PFDR_itMax=2000)
    # a vector A: the diagonal, obs and A premultiplied (obs * A, A * A)
    Cv, rX = pfdr.CP_quadratic_l1_duplex(y, p["Eu"].astype(np.uint32), p["Ev"].astype(np.uint32),
                                         0.3, a, 0.02, **kw)
    q = dict(p, Y=(y * a).astype(F32), A=(a * a).astype(F32), CP_itMax=4)
    want = entry("duplex", q)
    assert Cv.dtype == np.uint32 and np.array_equal(Cv, want[0]) and same_bytes(rX, want[1])
    # a scalar A: the identity, its value discarded
    Cv, rX = pfdr.CP_quadratic_l1_duplex(y, p["Eu"], p["Ev"], p["La_d1"], 3.0, p["La_l1"], **kw)
    want = entry("duplex", dict(p, Y=y, A=None, CP_itMax=4))
    assert np.array_equal(Cv, want[0]) and same_bytes(rX, want[1])
