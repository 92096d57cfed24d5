"""GPU: the operator norm (power method on the stored entries) and the
diagonal Lipschitz metric of a sparse A (CSC).

The yardsticks are numpy's: ||A||_2^2 from the SVD of the float64 matrix, at
the settings and tolerances of tests/test_gram_gpu.py's
test_operator_norm_matches_svd (nTol 1e-6, nbInit 10, relative error <= 1e-4
in f32 and <= 1e-5 in f64), and the float64 formula of the metric.  All
matrices are non-negative with a spectral gap sigma_2^2 / sigma_1^2 <= 0.48; the
numpy restatement of the batched power method with the same starts
(tests/power_twin.py, run on these matrices by tests/test_power_twin_cpu.py's
test_twin_matches_svd) is within 2.1e-6 (f32) and 3.0e-7 (f64) of the SVD on
every one of them, so the tolerances leave the algorithm itself a margin of
30x and more.  tests/test_power_method_gpu.py holds the entries to that
restatement's bytes, start by start, on signed matrices.
"""
import functools

import numpy as np
import pytest

import test_sparse_gpu as TS
from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

DTS = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
# name -> (N, V, density, itMax)
CASES = {"base": (300, 200, 0.1, 200), "longrows": (64, 5000, 0.1, 200),
         "longcols": (2000, 64, 0.1, 400), "holes": (257, 129, 0.05, 200),
         "onerow": (8, 20000, 0.002, 200)}


def _svd_tol(dt):
    return 1e-4 if dt == np.float32 else 1e-5


@functools.lru_cache(maxsize=None)
def _matrix(name, signed=False):
    """(A float64 N-by-V, mask of its random pattern, ||A||_2^2)"""
    N, V, dens = {"one_it": (40, 30, 0.2)}.get(name, CASES.get(name, (0,) * 4)[:3])
    rng = np.random.default_rng(5)
    A = rng.random((N, V))
    if signed:
        A = 2.0 * A - 1.0
    mask = rng.random((N, V)) < dens
    A = A * mask
    if name == "holes":  # an empty column, an empty row, sizes off every block boundary
        A[:, 7] = 0.0
        A[100, :] = 0.0
    if name == "onerow":  # one row of 20,000 entries
        A[3, :] = np.random.default_rng(9).random(V) + 0.1
    A.setflags(write=False)
    return A, mask, float(np.linalg.norm(A, 2) ** 2)


@functools.lru_cache(maxsize=None)
def _csc(name, dtname, signed=False):
    return pfdr.CSC.from_dense(_matrix(name, signed)[0].astype(dtname))


@functools.lru_cache(maxsize=None)
def _norm(name, dtname, nbInit=10, itMax=None):
    """computed once, shared by the tests that compare it"""
    itMax = CASES[name][3] if itMax is None else itMax
    return pfdr.operator_norm(_csc(name, dtname), nTol=1e-6, itMax=itMax, nbInit=nbInit)[0]


def _bits(x, dt):
    return np.asarray(x, dt).tobytes()


# ------------------------------------------------------- 1. against the SVD --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(CASES))
def test_matches_svd(gpu_lib, name, dt):
    exact = _matrix(name)[2]
    got = _norm(name, np.dtype(dt).name)
    rel = abs(got - exact) / exact
    print("%s %s: norm2 %.9g, SVD %.9g, relative error %.3e" % (name, np.dtype(dt).name, got,
                                                                exact, rel))
    assert rel <= _svd_tol(dt), (name, got, exact, rel)


# ------------------------------------------------------------ 2. one iteration --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_one_iteration_is_a_lower_estimate(gpu_lib, dt):
    exact = _matrix("one_it")[2]
    got = pfdr.operator_norm(_csc("one_it", np.dtype(dt).name), nTol=1e-6, itMax=1, nbInit=10)[0]
    print("one iteration %s: %.9g = %.4f of the SVD's" % (np.dtype(dt).name, got, got / exact))
    assert 0 < got <= exact * (1 + 1e-5), (got, exact)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_negative_itmax_runs_no_iteration(gpu_lib, dt):
    """as the dense entry: the estimate after the first product alone"""
    exact = _matrix("one_it")[2]
    csc = _csc("one_it", np.dtype(dt).name)
    got = pfdr.operator_norm(csc, nTol=1e-6, itMax=-1, nbInit=10)[0]
    assert 0 < got <= exact * (1 + 1e-5), (got, exact)
    assert _bits(got, dt) == _bits(pfdr.operator_norm(csc, nTol=1e-6, itMax=0, nbInit=10)[0], dt)


# ------------------------------------------------------- 3. starts and batches --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_starts_and_batches(gpu_lib, dt):
    """nbInit 1, 10 -> a batch of 16; 17 -> 32; 33 -> 64; 70 -> two batches of
    64.  Each result is the maximum over a superset of the same per-start
    values, so they ascend exactly, unless a start's arithmetic depends on the
    batch it runs in."""
    exact = _matrix("base")[2]
    got = [_norm("base", np.dtype(dt).name, nbInit=n) for n in (1, 10, 17, 33, 70)]
    print(np.dtype(dt).name, ["%.9g" % g for g in got])
    for g in got:
        assert abs(g - exact) / exact <= _svd_tol(dt), (got, exact)
    assert all(a <= b for a, b in zip(got, got[1:])), got
    # nbInit <= 0 counts as 1
    assert _bits(_norm("base", np.dtype(dt).name, nbInit=0), dt) == _bits(got[0], dt)


# --------------------------------------------------------------- 4. same bytes --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_same_bytes(gpu_lib, dt):
    dtname = np.dtype(dt).name
    csc = _csc("base", dtname)
    ref = _bits(_norm("base", dtname), dt)
    kw = dict(nTol=1e-6, itMax=200, nbInit=10)
    assert _bits(pfdr.operator_norm(csc, **kw)[0], dt) == ref  # a second call
    assert _bits(pfdr.operator_norm(csc.to_device(), **kw)[0], dt) == ref
    A, mask, _ = _matrix("base")
    A = A.astype(dt)
    stored = A != 0
    free = np.argwhere(~stored)[37]
    stored[free[0], free[1]] = True  # a stored zero
    withzero = pfdr.CSC.from_dense(A, stored=stored)
    assert withzero.nnz == csc.nnz + 1
    assert _bits(pfdr.operator_norm(withzero, **kw)[0], dt) == ref
    Lz, bz = pfdr.lipschitz_diag(withzero)
    L, b = pfdr.lipschitz_diag(csc)
    assert Lz.tobytes() == L.tobytes() and _bits(bz, dt) == _bits(b, dt)


# -------------------------------------------------------------- 5. zero matrix --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_zero_matrix(gpu_lib, dt):
    csc = pfdr.CSC(np.array([0, 0, 1, 1, 1]), np.array([2]), np.zeros(1, dt), 4)
    got = pfdr.operator_norm(csc, nTol=1e-6, itMax=20, nbInit=10)[0]
    assert got == 0.0 and not np.signbit(got)
    L, bound = pfdr.lipschitz_diag(csc)
    assert not L.any() and bound == 0.0


# ----------------------------------------------------------- 6. malformed CSC --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_malformed_csc_is_refused_and_the_next_call_succeeds(gpu_lib, dt):
    dtname = np.dtype(dt).name
    good = _csc("base", dtname)
    v = int(np.argmax(np.diff(good.colptr) >= 2))
    e = int(good.colptr[v])
    descending = good.rowidx.copy()
    descending[[e, e + 1]] = descending[[e + 1, e]]
    past = good.rowidx.copy()
    past[e] = good.N
    short = good.colptr.copy()
    short[-1] -= 1
    bad = [(pfdr.CSC(good.colptr, descending, good.val, good.N), "strictly ascending"),
           (pfdr.CSC(good.colptr, past, good.val, good.N), "row index outside"),
           (pfdr.CSC(short, good.rowidx, good.val, good.N), "colptr")]
    for csc, needle in bad:
        with pytest.raises(pfdr.PFDRError, match=needle):
            pfdr.operator_norm(csc, nTol=1e-6, itMax=200, nbInit=10)
        with pytest.raises(pfdr.PFDRError, match=needle):
            pfdr.lipschitz_diag(csc)
        with pytest.raises(pfdr.PFDRError, match=needle):
            pfdr.operator_norm(csc.to_device(), nTol=1e-6, itMax=200, nbInit=10)
    assert _bits(pfdr.operator_norm(good, nTol=1e-6, itMax=200, nbInit=10)[0], dt) == _bits(
        _norm("base", dtname), dt)
    assert pfdr.lipschitz_diag(good)[0].shape == (good.V,)


# ---------------------------------------------------------- 7. diagonal metric --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name,signed", [("base", False), ("base", True), ("holes", False)],
                         ids=["base", "signed", "holes"])
def test_diagonal_metric(gpu_lib, name, signed, dt):
    """L and bound against the float64 formula: one rounding to nearest (2^-24
    in f32) plus the double sums' error -> 1.2e-7 per entry in f32, 1e-14 in
    f64; diag(L) - A^tA is positive semi-definite up to rounding (measured on
    the CPU: -4.6e-10 max L on the non-negative case, where Cauchy-Schwarz is
    tight); ||A||^2 <= max L <= bound."""
    dtname = np.dtype(dt).name
    csc = _csc(name, dtname, signed)
    A = _matrix(name, signed)[0].astype(dt).astype(np.float64)
    exact = float(np.linalg.norm(A, 2) ** 2)
    absA = np.abs(A)
    r = absA.sum(axis=1)
    Lref = absA.T @ r
    bref = absA.sum(axis=0).max() * r.max()
    tol = 1.2e-7 if dt == np.float32 else 1e-14
    L, bound = pfdr.lipschitz_diag(csc)
    assert L.dtype == dt and L.shape == (csc.V,)
    L64 = L.astype(np.float64)
    err = np.abs(L64 - Lref) / np.where(Lref > 0, Lref, 1.0)
    print("%s %s: worst relative error of L %.3e, of bound %.3e" % (
        name, dtname, err.max(), abs(float(bound) - bref) / bref))
    assert err.max() <= tol, err.max()
    assert abs(float(bound) - bref) <= tol * bref, (bound, bref)
    if name == "holes":
        assert L[7] == 0
    floor = -1e-6 if dt == np.float32 else -1e-12
    low = float(np.linalg.eigvalsh(np.diag(L64) - A.T @ A).min())
    print("  smallest eigenvalue of diag(L) - AtA: %.3e max L" % (low / L64.max()))
    assert low >= floor * L64.max(), (low, L64.max())
    assert exact <= L64.max() * (1 + 1e-6) <= float(bound) * (1 + 1e-6), (exact, L64.max(), bound)
    # a device CSC: the same bytes, in a tensor beside its arrays
    Ld, bd = pfdr.lipschitz_diag(csc.to_device())
    assert Ld.is_cuda and Ld.cpu().numpy().tobytes() == L.tobytes()
    assert _bits(bd, dt) == _bits(bound, dt)


def test_bound_is_the_front_ends_numpy_bound(gpu_lib):
    """byte for byte: both add the stored entries in stored order in double"""
    for dt in DTS:
        for signed in (False, True):
            csc = _csc("base", np.dtype(dt).name, signed)
            a = np.abs(csc.val.astype(np.float64))
            cols = np.repeat(np.arange(csc.V), np.diff(csc.colptr))
            nb = np.array([np.bincount(cols, a, csc.V).max() *
                           np.bincount(csc.rowidx, a, csc.N).max()], dt)
            assert _bits(pfdr.lipschitz_diag(csc)[1], dt) == nb.tobytes()


# --------------------------------------------------- 8. sessions take the metric --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_sparse_session_with_the_diagonal_metric(gpu_lib, oracle_port, monkeypatch, dt):
    """tests/test_sparse_gpu.py's small case (20 x 15 grid, N = 200), Ltype =
    DIAG with L = lipschitz_diag(csc)[0], 40 fixed iterations: X and it are the
    restatement's bytes on the densified matrix with the same L."""
    monkeypatch.delenv("PFDR_SPARSE_EXACT", raising=False)
    p = TS._problem("a", np.dtype(dt).name)
    V, K = p["V"], 40
    L = pfdr.lipschitz_diag(p["csc"])[0]
    assert L.shape == (V,) and (L > 0).all()
    ref = oracle_port.quadratic_d1_l1(np.zeros(V, dt), p["Y"], p["Acm"], p["N"], p["Eu"], p["Ev"],
                                      p["La_d1"], La_l1=p["La_l1"], positivity=0, Ltype=pfdr.DIAG,
                                      L=L, rho=1.5, condMin=1e-3, difRcd=0.0, difTol=0.0, itMax=K)
    s = pfdr.Session(pfdr.PFDR_KIND_L1, dt, V, p["Eu"].size, N=p["N"], A=p["csc"], Eu=p["Eu"],
                     Ev=p["Ev"], La_d1=p["La_d1"], La_l1=p["La_l1"], X0=np.zeros(V, dt), Y=p["Y"],
                     Ltype=pfdr.DIAG, L=L, rho=1.5, condMin=1e-3, difRcd=0.0, difTol=0.0, itMax=K)
    try:
        s.run(K)
        X, it = s.result()[:2]
        assert s.query("sparse_exact") == 1
    finally:
        s.close()
    assert it == ref[1] == K
    assert X.tobytes() == ref[0].tobytes(), TS._rel_l2(X, ref[0])


# ------------------------------------------------------------------ 9. front end --
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_front_end_choices(gpu_lib, dt):
    p = TS._problem("a", np.dtype(dt).name)
    V, K = p["V"], 40
    front = lambda **kw: pfdr.PFDR_quadratic_l1(p["Y"], p["Eu"], p["Ev"], p["La_d1"], p["csc"],
                                                p["La_l1"], PFDR_itMax=K, PFDR_difTol=0, **kw)
    direct = lambda Ltype, L: gpu_lib.quadratic_d1_l1(
        np.zeros(V, dt), p["Y"], p["csc"], p["N"], p["Eu"], p["Ev"], p["La_d1"], La_l1=p["La_l1"],
        positivity=0, Ltype=Ltype, L=L, rho=1.0, condMin=1e-3, difRcd=0.0, difTol=0.0, itMax=K)[:2]
    x, it = front(lipschitz="power")
    xd, itd = direct(pfdr.SCAL, np.array([pfdr.operator_norm(p["csc"])[0]], dt))
    assert it == itd == K and x.tobytes() == xd.tobytes()
    x, it = front(lipschitz="diag")
    xd, itd = direct(pfdr.DIAG, pfdr.lipschitz_diag(p["csc"])[0])
    assert it == itd == K and x.tobytes() == xd.tobytes()
    x, it = front()
    xb, itb = front(lipschitz="bound")
    assert it == itb == K and x.tobytes() == xb.tobytes()
    xd, itd = direct(pfdr.SCAL, np.array([pfdr.lipschitz_diag(p["csc"])[1]], dt))
    assert x.tobytes() == xd.tobytes()


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_front_end_iterations_are_reported(gpu_lib, dt):
    """A measurement, not an order: the iterations to difTol = 1e-4 under the
    three choices on the signed 300 x 200 operator (a chain graph)."""
    dtname = np.dtype(dt).name
    csc = _csc("base", dtname, True)
    A = _matrix("base", True)[0]
    rng = np.random.default_rng(6)
    x0 = np.where(rng.random(csc.V) < 0.5, 1.0, -0.5)
    Y = (A @ x0 + 0.05 * (rng.random(csc.N) - 0.5)).astype(dt)
    Eu, Ev = TS._chain(csc.V)
    for choice in ("bound", "power", "diag"):
        x, it = pfdr.PFDR_quadratic_l1(Y, Eu, Ev, 0.05, csc, 0.01, lipschitz=choice,
                                       PFDR_itMax=20000)
        print("%s lipschitz=%s: %d iterations to difTol 1e-4" % (dtname, choice, it))
        assert 0 < it <= 20000 and np.isfinite(x).all()
