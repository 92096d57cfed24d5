"""numpy restatements of the two batched power methods (pfdr_operator_norm_*,
pfdr_operator_norm_csc_*) and of the sparse diagonal metric
(pfdr_lipschitz_diag_csc_*).  Imported by tests, not collected.

Everything is vectorised over the starts: a function returns the vector of
per-start results b[0 .. starts - 1], and the library's answer for nbInit = n
is best(b, n).  The library is built with -ffp-contract=off, correctly rounded
division and square root and no flushing of subnormals, so + - * / sqrt in
float32 and float64 round as numpy's do and sparse_exact / lipschitz_exact
reproduce its bytes; plain is the same iteration with numpy's products and
norms, the yardstick of the dense entry, whose summation order is no contract.
"""
import numpy as np

NORM_LANES = 16    # kNormLanes of csrc/pfdr_sparse_norm.hip
NORM_ROWS = 1024   # kNormRows
MUTATIONS = ("batch_restart", "lanes_desc", "products_desc", "drop_tail")


def start_value(i):
    """power_start_value (csrc/pfdr_power.hpp) of the numbers i, in double"""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = np.asarray(i, u) * u(0xD1B54A32D192ED03) + u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    return (z >> u(11)).astype(np.float64) * (1.0 / 9007199254740992.0) * 2.0 - 1.0


def start_block(n, numbers, dt):
    """X (n x len(numbers)): coordinate r of start number c is value r + c n"""
    r = np.arange(n, dtype=np.uint64)[:, None]
    c = np.asarray(numbers, np.uint64)[None, :]
    with np.errstate(over="ignore"):
        return start_value(r + c * np.uint64(n)).astype(dt)


def batch_width(starts):
    return 16 if starts <= 16 else 32 if starts <= 32 else 64


def best(b, n, dt):
    """max(b[:n]) as the entries take it: from +0.0, NaN never wins"""
    out = np.zeros((), dt)
    for x in np.asarray(b[:max(n, 1)], dt):
        if x > out:
            out = x
    return dt(out)


def prefix_best(b, dt):
    """best(b, n) for n = 1 .. len(b)"""
    v = np.where(np.asarray(b, dt) > 0, np.asarray(b, dt), dt(0))  # NaN > 0 is false
    return np.maximum.accumulate(v)


def records(b):
    """the record-setting starts c: b[c] > max(b[:c]) (from +0.0)"""
    p = prefix_best(b, np.asarray(b).dtype.type)
    return [c for c in range(len(p)) if p[c] > (p[c - 1] if c else 0)]


def iterate(X, step, norm, dt, nTol, itMax):
    """The iteration both entries share.  Returns (b, at): at[c] = the iteration
    at which start c stopped, -1 where it ran to the end."""
    nTol = dt(nTol)
    with np.errstate(all="ignore"):
        b = norm(X)
        X = step(X / b)
        b = norm(X)
        stopped = np.zeros(b.shape, bool)
        at = np.full(b.shape, -1)
        for it in range(max(itMax, 0)):
            X = step(X / b)  # stopped starts go on being divided by their frozen b
            a = norm(X)
            stop = ~stopped & ((a - b) / b < nTol)
            upd = ~stopped & ~stop
            stopped |= stop
            at[stop] = it
            b = np.where(upd, a, b)
            if not upd.any():
                break
    assert b.dtype == dt and X.dtype == dt
    return b, at


def plain(apply, n, dt, nTol, itMax, starts, stops=False):
    """step given as a function (A.T @ (A @ X) or G @ X), numpy's norm"""
    dt = np.dtype(dt).type
    X = start_block(n, np.arange(starts), dt)
    b, at = iterate(X, apply, lambda Z: np.linalg.norm(Z, axis=0).astype(dt), dt, nTol, itMax)
    return (b, at) if stops else b


class _Segments:
    """out[r] = sum of val[e] * in[idx[e]] over segment r's entries, ascending,
    product rounded and then added -- all segments longer than k advance at
    once, for k = 0 .. the longest segment's length - 1"""

    def __init__(self, ptr, idx, val, mutate):
        self.nout = ptr.size - 1
        lens = np.diff(ptr)
        if mutate == "drop_tail":
            lens = lens - (lens % 8 == 1)
        order = np.argsort(-lens, kind="stable")
        sorted_lens = lens[order]
        self.steps = []
        for k in range(int(lens.max()) if lens.size else 0):
            sel = order[:int((sorted_lens > k).sum())]
            e = ptr[sel] + (lens[sel] - 1 - k if mutate == "products_desc" else k)
            self.steps.append((sel, val[e][:, None], idx[e]))

    def __call__(self, X):
        acc = np.zeros((self.nout, X.shape[1]), X.dtype)
        for sel, v, j in self.steps:
            acc[sel] += v * X[j]
        return acc


def _stage(Z, per, lanes_desc):
    """k_spn_colsum: block k takes rows k per .. k per + per - 1, lane j adds
    its rows j, j + 16, ... ascending, then the 16 lane sums are added in order"""
    n, S = Z.shape
    nb = -(-n // per)
    depth = -(-per // NORM_LANES)
    assert nb == 1 or per == depth * NORM_LANES
    Zp = np.zeros((nb * depth * NORM_LANES, S), Z.dtype)  # s + 0.0 = s for s >= +0.0
    Zp[:n] = Z
    Zp = Zp.reshape(nb, depth, NORM_LANES, S)
    s = np.zeros((nb, NORM_LANES, S), Z.dtype)
    for i in range(depth):
        s += Zp[:, i]
    lanes = range(NORM_LANES - 1, -1, -1) if lanes_desc else range(NORM_LANES)
    t = None
    for q in lanes:
        t = s[:, q].copy() if t is None else t + s[:, q]
    return t


def tree_norm(X, lanes_desc=False):
    """col_norms: the fixed two-stage tree of the sparse entry"""
    part = _stage(X * X, NORM_ROWS, lanes_desc)
    return np.sqrt(_stage(part, part.shape[0], lanes_desc)[0])


def csr_view(colptr, rowidx, val, N):
    """rows in order, columns ascending inside a row: a stable sort by row"""
    order = np.argsort(rowidx, kind="stable")
    cols = np.repeat(np.arange(colptr.size - 1), np.diff(colptr))
    rowptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(rowidx, minlength=N), out=rowptr[1:])
    return rowptr, cols[order], val[order]


def sparse_exact(csc, dt, nTol, itMax, starts, mutate=None, stops=False):
    """pfdr_operator_norm_csc_*'s per-start results, bit for bit, all arithmetic
    in dt.  mutate names one deliberate error (MUTATIONS), for the tests that
    show that a byte comparison would notice it."""
    assert mutate is None or mutate in MUTATIONS
    dt = np.dtype(dt).type
    colptr = np.asarray(csc.colptr, np.int64)
    rowidx = np.asarray(csc.rowidx, np.int64)
    val = np.asarray(csc.val).astype(dt)
    rowptr, colidx, rval = csr_view(colptr, rowidx, val, csc.N)
    AX = _Segments(rowptr, colidx, rval, mutate)     # T = A X over the CSR view
    AtT = _Segments(colptr, rowidx, val, mutate)     # Y = A^t T over the CSC as stored
    numbers = np.arange(starts)
    if mutate == "batch_restart":
        numbers = numbers % batch_width(starts)
    X = start_block(csc.V, numbers, dt)
    b, at = iterate(X, lambda Z: AtT(AX(Z)), lambda Z: tree_norm(Z, mutate == "lanes_desc"), dt,
                    nTol, itMax)
    return (b, at) if stops else b


def lipschitz_exact(csc):
    """pfdr_lipschitz_diag_csc_*'s (L, bound), bit for bit: double sums in
    stored order (np.bincount adds sequentially), rounded once"""
    dt = np.dtype(csc.dtype).type
    colptr = np.asarray(csc.colptr, np.int64)
    rowidx = np.asarray(csc.rowidx, np.int64)
    a = np.abs(np.asarray(csc.val).astype(np.float64))
    cols = np.repeat(np.arange(csc.V), np.diff(colptr))
    r = np.bincount(rowidx, a, csc.N)
    L = np.bincount(cols, a * r[rowidx], csc.V).astype(dt)
    colsum = np.bincount(cols, a, csc.V)
    return L, dt(colsum.max() * r.max())
