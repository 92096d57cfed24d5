"""GPU: both power methods and the sparse diagonal metric against their numpy
restatements (tests/power_twin.py), start by start.

Sparse entry and metric: the bytes of the twin.  pfdr_operator_norm_csc_* adds
every row, column and norm sum in a fixed, documented order in the real type,
so operator_norm(csc, nbInit=n) is max(sparse_exact(...)[:n]) bit for bit;
lipschitz_diag is np.bincount's sums in double, rounded once.  The per-start
values are seen through the prefix maxima alone, which is why
tests/test_power_twin_cpu.py asserts that the sweep matrix sets a record in
every batch and that each of four kernel errors (a second batch that repeats
the first one's starts, the norm's lane sums or a segment's products added in
the other order, a dropped tail entry) changes a compared result.

Dense entry: its summation order (split contraction, wave tree, the Gram
matrix when the cost model takes it) is no contract, so it is held to the
float64 run of the same iteration with the same starts: 1e-12 relative in f64;
in f32, 8 x the deviation of numpy's own float32 run of that iteration from
its float64 run over all these cases (measured 9.0e-7, so 7.2e-6: PC.dense_tol,
re-measured where the tests run), 100 x below the >= 1e-3 by which the
tail matrix's best start, the 65th, beats the first 64.
"""
import numpy as np
import pytest

import power_cases as PC
import power_twin as PT
from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

DTS, DT_IDS = PC.DTS, PC.DT_IDS


def _sparse_mismatches(name, dt, settings, ns, device=False):
    """the (nTol, itMax, n) at which operator_norm's bytes are not the twin's"""
    dtname = np.dtype(dt).name
    csc = PC.csc(name, dtname)
    if device:
        csc = csc.to_device()
    bad = []
    for nTol, itMax in settings:
        b = PC.sparse_twin(name, dtname, nTol, itMax)[0]
        for n in ns:
            got = dt(pfdr.operator_norm(csc, nTol=nTol, itMax=itMax, nbInit=n)[0])
            want = PT.best(b, n, dt)
            if got.tobytes() != want.tobytes():
                bad.append((nTol, itMax, n, float(got), float(want)))
    return bad


PLAIN = ((1e-6, -1), (1e-6, 3))


# ------------------------------------------------------------------ sparse --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_sparse_sweep_every_number_of_starts(gpu_lib, dt):
    bad = _sparse_mismatches("sweep", dt, PLAIN, range(1, 71))
    assert not bad, bad[:5]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", ["lengths", "longrow"] + ["tree%d" % V for V in PC.TREE_V])
def test_sparse_bytes(gpu_lib, name, dt):
    bad = _sparse_mismatches(name, dt, PLAIN, PC.NS)
    assert not bad, bad[:5]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_sparse_stopping_rule(gpu_lib, dt):
    """starts that stop at iterations 3 .. 7, none that stops, all at once"""
    bad = _sparse_mismatches("sweep", dt, ((0.02, 60), (-1.0, 4), (1e30, 3)), PC.NS)
    assert not bad, bad[:5]


def test_sparse_subnormal_f32(gpu_lib):
    bad = _sparse_mismatches("subnormal", np.float32, PLAIN, PC.NS)
    assert not bad, bad[:5]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_sparse_nan_entry(gpu_lib, dt):
    for n in (1, 17, 70):
        assert PT.best(PC.sparse_twin("nan", np.dtype(dt).name, 1e-6, 3)[0], n, dt) == 0
        got = pfdr.operator_norm(PC.csc("nan", np.dtype(dt).name), nTol=1e-6, itMax=3, nbInit=n)[0]
        assert got == 0.0 and not np.signbit(got), got


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_sparse_device_csc(gpu_lib, dt):
    bad = _sparse_mismatches("lengths", dt, PLAIN, PC.NS, device=True)
    assert not bad, bad[:5]


# ----------------------------------------------------------- sparse metric --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", ["sweep", "lengths", "nonneg"])
def test_metric_bytes(gpu_lib, name, dt):
    csc = PC.csc(name, np.dtype(dt).name)
    Lref, bref = PT.lipschitz_exact(csc)
    L, bound = pfdr.lipschitz_diag(csc)
    assert L.dtype == dt and L.tobytes() == Lref.tobytes(), np.flatnonzero(L != Lref)[:5]
    assert dt(bound).tobytes() == bref.tobytes(), (bound, bref)
    Ld, bd = pfdr.lipschitz_diag(csc.to_device())
    assert Ld.is_cuda and Ld.cpu().numpy().tobytes() == Lref.tobytes()
    assert dt(bd).tobytes() == bref.tobytes(), (bd, bref)


# ------------------------------------------------------------------- dense --
def _dense_check(name, dt, symmetric=False):
    dtname = np.dtype(dt).name
    A = PC.dense_input(name, dtname)
    tol = PC.dense_tol(dt)
    worst, bad = 0.0, []
    for itMax in PC.DENSE[name][3]:
        want = PT.prefix_best(PC.dense_twin(name, dtname, itMax)[0], np.float64)
        for n in PC.DENSE_NS:
            got = pfdr.operator_norm(A, nTol=PC.DENSE_NTOL, itMax=itMax, nbInit=n,
                                     symmetric=symmetric)[0]
            rel = abs(float(got) - want[n - 1]) / want[n - 1]
            worst = max(worst, rel)
            if not rel <= tol:
                bad.append((itMax, n, float(got), float(want[n - 1]), rel))
    print("%s %s: worst relative deviation %.3e (allowed %.3e)" % (name, dtname, worst, tol))
    assert not bad, bad[:5]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", ["tail", "odd", "narrow", "split", "wide3", "wide"])
def test_dense_against_the_float64_iteration(gpu_lib, name, dt):
    _dense_check(name, dt)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", ["sym200", "sym1100"])
def test_dense_symmetric_input(gpu_lib, name, dt):
    _dense_check(name, dt, symmetric=True)


@pytest.mark.parametrize("name", ["tail", "wide"])
def test_dense_and_sparse_entries_share_their_starts(gpu_lib, name):
    """f64, no iteration after the first product: sums of <= 300 terms, 300 x
    1.1e-16 x a conditioning factor of ~10 is well under 1e-12"""
    A = PC.dense_input(name, "float64")
    csc = pfdr.CSC.from_dense(A)
    for n in PC.DENSE_NS:
        dense = pfdr.operator_norm(A, nTol=1e-6, itMax=0, nbInit=n)[0]
        sparse = pfdr.operator_norm(csc, nTol=1e-6, itMax=0, nbInit=n)[0]
        assert abs(dense - sparse) <= 1e-12 * sparse, (n, dense, sparse)
