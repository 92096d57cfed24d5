"""CPU: the numpy restatements of the power methods (tests/power_twin.py) are
right, and the inputs of tests/test_power_method_gpu.py have teeth.

1. The twin at the settings of tests/test_sparse_opnorm_gpu.py is within a
   tenth of that file's tolerance of the SVD, so a byte comparison with the
   twin asks no less than that file does.
2. The per-start results are seen only through prefix maxima, so the sweep
   matrices must set records in every batch, the dense tail matrix must have
   its best start past the 64th, and the stop and subnormal cases must do what
   their names say: asserted here, so that an edited seed cannot blunt the GPU
   tests unnoticed.
3. Four deliberate errors in the exact twin (the kernel errors a tolerance
   against the SVD cannot see) each change the bytes of a compared result.
"""
import numpy as np
import pytest

import power_cases as PC
import power_twin as PT
import test_sparse_opnorm_gpu as SO
from cp_pfdr_graph_d1_amd import pfdr

DTS, DT_IDS = PC.DTS, PC.DT_IDS


# ------------------------------------------------------- 1. against the SVD --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_twin_matches_svd(dt):
    dtname = np.dtype(dt).name
    worst = 0.0
    for name, (_, _, _, itMax) in SO.CASES.items():
        A, _, exact = SO._matrix(name)
        A = A.astype(dt)
        if name == "onerow":  # a 20,000-entry row is too slow in order
            b = PT.plain(lambda X: A.T @ (A @ X), A.shape[1], dt, 1e-6, itMax, 10)
        else:
            b = PT.sparse_exact(pfdr.CSC.from_dense(A), dt, 1e-6, itMax, 10)
        rel = abs(float(PT.best(b, 10, dt)) - exact) / exact
        print("%s %s: twin within %.3e of the SVD" % (name, dtname, rel))
        worst = max(worst, rel)
    print("%s: worst relative error %.3e" % (dtname, worst))
    assert worst <= SO._svd_tol(dt) / 10, worst


def test_start_values():
    """the first values by hand: splitmix64's finaliser on i * odd + golden"""
    def one(i):
        m = (1 << 64) - 1
        z = (i * 0xD1B54A32D192ED03 + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return (z >> 11) * 2.0 ** -53 * 2.0 - 1.0
    i = [0, 1, 2, 97 * 131, 70 * 17413 + 5, 2 ** 40 + 3]
    assert PT.start_value(np.array(i, np.uint64)).tolist() == [one(k) for k in i]
    X = PT.start_block(5, [0, 3, 64], np.float32)
    assert X.dtype == np.float32 and X[2, 1] == np.float32(one(2 + 3 * 5))
    assert X[4, 2] == np.float32(one(4 + 64 * 5))


def test_exact_twin_is_the_plain_twin_up_to_rounding():
    """the ordered products and the norm tree restate A^t(A X) and ||.||"""
    A = PC.sweep()
    exact = PT.sparse_exact(PC.csc("sweep", "float64"), np.float64, 1e-6, 3, PC.STARTS)
    plain = PT.plain(lambda X: A.T @ (A @ X), A.shape[1], np.float64, 1e-6, 3, PC.STARTS)
    assert np.max(np.abs(exact - plain) / plain) <= 1e-13


# -------------------------------------------- 2. conditions on the matrices --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_sweep_sets_a_record_in_every_batch(dt):
    rec = PT.records(PC.sparse_twin("sweep", np.dtype(dt).name, 1e-6, -1)[0])
    print(np.dtype(dt).name, "records", rec)
    for lo, hi in ((16, 32), (32, 64), (64, 70)):
        assert any(lo <= c < hi for c in rec), (lo, hi, rec)


@pytest.mark.parametrize("itMax", [0, 2])
def test_dense_tail_has_its_best_start_past_the_64th(itMax):
    b = PC.dense_twin("tail", "float64", itMax)[0]
    gap = b[64:70].max() / b[:64].max() - 1
    print("itMax %d: tail over head %.3e, best start %d" % (itMax, gap, int(np.argmax(b))))
    assert gap >= 1e-3, gap


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_stop_case_stops_at_several_iterations(dt):
    dtname = np.dtype(dt).name
    at = PC.sparse_twin("sweep", dtname, 0.02, 60)[1]
    print(dtname, "stops at", sorted(set(at.tolist())))
    assert (at >= 0).all() and len(set(at.tolist())) >= 3
    assert (PC.sparse_twin("sweep", dtname, -1.0, 4)[1] == -1).all()
    b, at = PC.sparse_twin("sweep", dtname, 1e30, 3)
    assert (at == 0).all()  # at once, keeping the first product's norm
    assert b.tobytes() == PC.sparse_twin("sweep", dtname, 1e-6, -1)[0].tobytes()


def test_subnormal_case_uses_subnormal_arithmetic():
    for itMax in (-1, 3):
        b = PC.sparse_twin("subnormal", "float32", 1e-6, itMax)[0]
        scaled = PC.sparse_twin("sweep", "float32", 1e-6, itMax)[0] * np.float32(2.0 ** -64)
        assert np.isfinite(b).all() and (b > 0).all()
        assert b.tobytes() != scaled.tobytes()
        # ... and in a result that the GPU test compares
        hit = [n for n in PC.NS
               if PT.best(b, n, np.float32).tobytes() != PT.best(scaled, n, np.float32).tobytes()]
        print("itMax %d: %d of %d starts differ from the scaled results, nbInit %s see it" % (
            itMax, int((b != scaled).sum()), b.size, hit))
        assert hit


def test_no_dense_start_stops():
    """so the dense comparison never hangs on a stopping decision that the
    last bit of a norm could turn"""
    for name, (_, _, _, its) in PC.DENSE.items():
        for itMax in its:
            for dtname, twin in (("float32", "float32"), ("float32", "float64"),
                                 ("float64", "float64")):
                assert (PC.dense_twin(name, dtname, itMax, twin)[1] == -1).all(), (name, itMax)


def test_dense_f32_allowance():
    dev = PC.dense_f32_deviation()
    print("float32 plain() against float64 plain(): worst prefix maximum off by %.3e; "
          "the GPU is allowed %.3e" % (dev, PC.dense_tol(np.float32)))
    assert 0 < dev and PC.dense_tol(np.float32) == 8 * dev
    assert PC.dense_tol(np.float32) * 100 <= 1e-3  # the gaps the dense tests rely on


# ------------------------------------------------------------ 3. sensitivity --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("mutate", PT.MUTATIONS)
def test_a_byte_comparison_notices(mutate, dt):
    dtname = np.dtype(dt).name
    seen = []
    for name in ("sweep", "lengths", "longrow"):
        for itMax in (-1, 3):
            good = PC.sparse_twin(name, dtname, 1e-6, itMax)[0]
            bad = PC.sparse_twin(name, dtname, 1e-6, itMax, mutate)[0]
            ns = range(1, 71) if name == "sweep" else PC.NS
            hit = [n for n in ns if PT.best(good, n, dt).tobytes() != PT.best(bad, n, dt).tobytes()]
            if hit:
                seen.append((name, itMax, hit))
    print(mutate, dtname, seen)
    assert seen, "%s (%s) changes no compared result on sweep, lengths or longrow" % (mutate, dtname)


def test_metric_twin_is_the_float64_formula():
    for name in ("sweep", "lengths", "nonneg"):
        for dt in DTS:
            csc = PC.csc(name, np.dtype(dt).name)
            A = np.abs(PC.MATRICES[name]().astype(dt).astype(np.float64))
            L, bound = PT.lipschitz_exact(csc)
            Lref = A.T @ A.sum(axis=1)
            bref = A.sum(axis=0).max() * A.sum(axis=1).max()
            tol = 1.2e-7 if dt == np.float32 else 1e-14
            assert L.dtype == dt and np.all(np.abs(L - Lref) <= tol * Lref)
            assert abs(float(bound) - bref) <= tol * bref
    assert PT.lipschitz_exact(PC.csc("lengths", "float64"))[0][160] == 0  # the empty column
