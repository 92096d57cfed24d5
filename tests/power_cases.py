"""The inputs of tests/test_power_twin_cpu.py and tests/test_power_method_gpu.py
and their twin results, computed once and shared.  Imported, not collected."""
import functools

import numpy as np

import power_twin as PT
from cp_pfdr_graph_d1_amd import pfdr

DTS = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
NS = (1, 2, 16, 17, 32, 33, 64, 65, 70)         # sparse: both sides of every batch width
DENSE_NS = (1, 10, 16, 17, 32, 33, 64, 65, 70)
STARTS = 70
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
TREE_V = (1, 15, 17, 1023, 1025, 2049, 16385, 17413)


def _ro(A):
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def random_matrix(N, V, seed):
    """signed, density 0.15"""
    rng = np.random.default_rng(seed)
    return _ro((2 * rng.random((N, V)) - 1) * (rng.random((N, V)) < 0.15))


def sweep():
    return random_matrix(97, 131, 5)


def dense_tail():
    return random_matrix(300, 131, 1)


@functools.lru_cache(maxsize=None)
def lengths_matrix():
    """177 x 177, block diagonal: rows 0 .. 16 hold exactly LENGTHS entries
    among the columns 0 .. 159, columns 160 .. 176 exactly LENGTHS entries
    among the rows 17 .. 176 -- row 0 and column 160 are empty"""
    rng = np.random.default_rng(11)
    blocks = []
    for _ in range(2):
        Bk = np.zeros((17, 160))
        for i, k in enumerate(LENGTHS):
            at = rng.choice(160, k, replace=False)
            Bk[i, at] = (0.25 + 0.75 * rng.random(k)) * rng.choice([-1.0, 1.0], k)
        blocks.append(Bk)
    A = np.zeros((177, 177))
    A[:17, :160] = blocks[0]
    A[17:, 160:] = blocks[1].T
    assert ((A != 0).sum(axis=1)[:17] == LENGTHS).all() and ((A != 0).sum(axis=0)[160:] == LENGTHS).all()
    return _ro(A)


@functools.lru_cache(maxsize=None)
def tree_csc(V, dtname):
    """two signed entries per column, N = 50 (3 for V = 1)"""
    N = 3 if V == 1 else 50
    rng = np.random.default_rng(100 + V)
    first = rng.integers(0, N, V)
    second = (first + 1 + rng.integers(0, N - 1, V)) % N
    rows = np.sort(np.stack([first, second], axis=1), axis=1).ravel()
    val = (0.25 + 0.75 * rng.random(2 * V)) * rng.choice([-1.0, 1.0], 2 * V)
    return pfdr.CSC(2 * np.arange(V + 1), rows, val.astype(dtname), N)


@functools.lru_cache(maxsize=None)
def longrow_matrix():
    """4 x 1100 with one full row: one group's loop over 69, 35 and 18 chunks"""
    A = np.array(random_matrix(4, 1100, 16))
    A[2, :] = 2 * np.random.default_rng(38).random(1100) - 1
    assert (A[2] != 0).all()
    return _ro(A)


@functools.lru_cache(maxsize=None)
def nan_matrix():
    A = np.array(sweep())
    i, j = np.argwhere(A != 0)[101]
    A[i, j] = np.nan
    return _ro(A)


@functools.lru_cache(maxsize=None)
def nonneg_matrix():
    return _ro(np.abs(random_matrix(97, 131, 8)))


MATRICES = {"sweep": sweep, "lengths": lengths_matrix, "longrow": longrow_matrix,
            "nan": nan_matrix, "nonneg": nonneg_matrix,
            "subnormal": lambda: sweep() * 2.0 ** -32}


@functools.lru_cache(maxsize=None)
def csc(name, dtname):
    """the host CSC of a named sparse case ("tree<V>" included)"""
    if name.startswith("tree"):
        return tree_csc(int(name[4:]), dtname)
    return pfdr.CSC.from_dense(MATRICES[name]().astype(dtname))


@functools.lru_cache(maxsize=None)
def sparse_twin(name, dtname, nTol, itMax, mutate=None):
    """(b[0 .. 69], the iteration at which each start stopped), read-only"""
    b, at = PT.sparse_exact(csc(name, dtname), dtname, nTol, itMax, STARTS, mutate=mutate,
                            stops=True)
    return _ro(b), _ro(at)


# ------------------------------------------------------------------- dense --
# name -> (M, N, seed, the itMax values); "sym<S>" is the S x S matrix A^tA of a
# (S + 50) x S matrix, given with symmetric=True
DENSE = {"tail": (300, 131, 1, (0, 2, 5)), "odd": (257, 255, 8, (0, 2, 5)),
         "narrow": (1000, 65, 16, (0, 2, 5)), "split": (2100, 1030, 38, (0, 2, 5)),
         "wide3": (40, 2100, 8, (0, -1)), "wide": (64, 300, 16, (0, -1)),
         "sym200": (250, 200, 5, (5,)), "sym1100": (1150, 1100, 5, (5,))}
DENSE_NTOL = 1e-6  # no start of any dense case stops within its itMax (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def dense_input(name, dtname):
    """what operator_norm is given, in the real type"""
    M, N, seed, _ = DENSE[name]
    A = random_matrix(M, N, seed).astype(dtname)
    if name.startswith("sym"):
        A64 = A.astype(np.float64)
        A = (A64.T @ A64).astype(dtname)
    return _ro(A)


@functools.lru_cache(maxsize=None)
def dense_twin(name, dtname, itMax, twin_dt="float64"):
    """plain() in twin_dt on the matrix as the entry receives it in dtname"""
    A = dense_input(name, dtname).astype(twin_dt)
    step = (lambda X: A @ X) if name.startswith("sym") else (lambda X: A.T @ (A @ X))
    b, at = PT.plain(step, A.shape[1], twin_dt, DENSE_NTOL, itMax, STARTS, stops=True)
    return _ro(b), _ro(at)


@functools.lru_cache(maxsize=None)
def dense_f32_deviation():
    """The largest relative deviation of any prefix maximum of plain() run in
    float32 from plain() run in float64, over every dense case and itMax."""
    worst = 0.0
    for name, (_, _, _, its) in DENSE.items():
        for itMax in its:
            p64 = PT.prefix_best(dense_twin(name, "float32", itMax)[0], np.float64)
            p32 = PT.prefix_best(dense_twin(name, "float32", itMax, "float32")[0], np.float32)
            worst = max(worst, float(np.max(np.abs(p32.astype(np.float64) - p64) / p64)))
    return worst


def dense_tol(dt):
    """f64: <= 2100 terms per sum, 2100 x 1.1e-16 x a conditioning factor of
    ~10 stays under 1e-12.  f32: 8 x the deviation of numpy's own float32 run
    (another summation order of the same O(sqrt(n) 2^-24) process)."""
    return 1e-12 if np.dtype(dt) == np.float64 else 8 * dense_f32_deviation()
