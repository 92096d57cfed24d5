"""The one-call cut pursuit (pfdr_cp_quadratic_d1_l1, csrc/pfdr_cutpursuit.hip)
pinned on every path of its loop: the l1 flavour's cases of the checks in
tests/cp_entry_checks.py, a. to f. there.
"""
import pytest

# the shared bodies' asserts report their values like a test module's
pytest.register_assert_rewrite("cp_entry", "cp_entry_checks")

import cp_entry_checks as K
import cp_run_cases as RC

pytestmark = pytest.mark.gpu

FL = "l1"
PATH_IDS = K.PATH_IDS[FL]
_ids = K.path_ids(PATH_IDS)


@pytest.mark.parametrize("name", K.FIXTURES[FL])
def test_entry_is_the_reference_run(gpu_lib, name):
    K.entry_is_the_reference_run(FL, name)


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_entry_is_the_twin(gpu_lib, kind, dt):
    K.entry_is_the_twin(FL, kind, dt)


@pytest.mark.parametrize("kind,dt", PATH_IDS, ids=_ids)
def test_obj_and_dif_at_every_iteration(gpu_lib, kind, dt):
    K.obj_and_dif_at_every_iteration(FL, kind, dt)


@pytest.mark.parametrize("name", ["cp_grid2d_l1_f32", "cp_knn_diag_l1pos_f64"])
def test_obj_and_dif_on_fixtures(gpu_lib, name):
    K.obj_and_dif_on_fixtures(FL, name)


@pytest.mark.parametrize("name", [n for n in RC.NAMES if n.startswith(("pos_diag", "nothing"))])
def test_recorded_run_exact(gpu_lib, name):
    K.recorded_run_exact(FL, name)


@pytest.mark.parametrize("kind", ["direct12", "direct160", "AtA"])
@pytest.mark.parametrize("d", ["f32", "f64"])
def test_recorded_run_functional(gpu_lib, kind, d):
    K.recorded_run_functional(FL, d, kind)


def test_optional_outputs(gpu_lib):
    K.optional_outputs_and_repeatability(FL)


def test_argument_errors(gpu_lib):
    K.argument_errors(FL)
