"""Inputs, references and the chunk plan for the Gram kernel tests
(csrc/pfdr_gram.hip: k_gram, k_gram_v, k_gram_b).  No GPU here: every
family asserts its own precondition, so a bad case fails on the CPU
(tests/test_gram_cases_cpu.py).

Conventions.  B is the P x K matrix whose rows are the Gram indices,
G = B B^t.  The matrix handed to pfdr.gram is A = B^t (K x P, which = 0,
G = A^t A) or A = B (P x K, which = 1, G = A A^t).  The Python entry passes
ld = M = A.shape[0], so the 16-byte load path is taken when M is a multiple
of 16 / itemsize: K steers it for which = 0, P for which = 1.
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
UNIT = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}   # unit roundoff u


def unit(dtype):
    return UNIT[np.dtype(dtype).name]


def to_A(B, which):
    return np.ascontiguousarray(B.T) if which == 0 else np.ascontiguousarray(B)


def rows_of(A, which):
    """B (rows = Gram indices) of the matrix handed to pfdr.gram"""
    return A.T if which == 0 else A


def vector_ld(A):
    """whether gram() takes the 16-byte load path for the host call of A"""
    return A.shape[0] % (16 // A.dtype.itemsize) == 0


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ----------------------------------------------------------------- plan --
def plan(P, K, dtype, split=True):
    """gram()'s chunk arithmetic restated (pfdr_gram.hip gram(), gram_slots,
    gram_block).  Used only to assert that a listed shape still exercises
    what its comment says; it decides no result."""
    f32 = np.dtype(dtype) == np.float32
    BT, BK = (128, 32) if f32 else (64, 16)
    split = bool(split) and f32
    target = 4096 if split else 2048
    nb = -(-P // BT)
    tiles = nb * (nb + 1) // 2
    nchunk = max(1, min(-(-target // tiles), -(-K // (4 * BK))))
    if nchunk > 8:
        nchunk = -(-nchunk // 8) * 8
    kchunk = -(-K // nchunk)
    kchunk = -(-kchunk // BK) * BK
    nchunk = -(-K // kchunk) if K > 0 else 1
    per_xcd = nchunk % 8 == 0
    blocks = nchunk * tiles if per_xcd else 8 * (-(-tiles // 8)) * nchunk
    return dict(nb=nb, tiles=tiles, nchunk=nchunk, kchunk=kchunk,
                last=K - (nchunk - 1) * kchunk, blocks=blocks,
                branch="chunk-per-xcd" if per_xcd else "eighths",
                tile="k_gram_b" if split else "exact")


# The shapes of the exact tests, as (P, K), with what each exercises and the
# plan figures that say so (asserted in test_gram_cases_cpu.py).  TWINS
# gives the other parities of the leading dimension: K for which = 0, P for
# which = 1 (a multiple of 4 loads 16 bytes at a time in both types, an odd
# one loads scalars in both; 530 and 130 are vector for f64 only).
SHAPES = [
    # (P, K)      f32 plan                          f64 plan
    ((1, 1),      dict(tiles=1, nchunk=1),          dict(tiles=1, nchunk=1)),      # smallest
    ((127, 17),   dict(tiles=1, nchunk=1),          dict(nchunk=1)),               # one tile, P and K tails
    ((129, 31),   dict(tiles=3, nchunk=1),          dict(nchunk=1)),               # K tail below BK = 32
    ((257, 33),   dict(tiles=6, nchunk=1),          dict(nchunk=1)),               # K tail above BK
    ((300, 64),   dict(tiles=6, nchunk=1, branch="eighths"), dict(nchunk=1)),      # 6 tiles over 8 XCD shares
    ((65, 530),   dict(nchunk=5, last=18),          dict(nchunk=12, last=2)),
    ((130, 1031), dict(tiles=3, nchunk=11),         dict(nchunk=22)),
    ((257, 1000), dict(tiles=6, nchunk=8, branch="chunk-per-xcd"),
                  dict(nchunk=16, branch="chunk-per-xcd")),
    ((128, 2560), dict(tiles=1, nchunk=20, branch="eighths"), dict()),             # > 8, no multiple of 8
    ((129, 2561), dict(tiles=3, nchunk=21, last=1), dict()),                       # last chunk of one
    ((385, 1300), dict(tiles=10, nchunk=14),        dict()),
]
TWINS = {
    (1, 1): dict(K=[4], P=[4]),
    (127, 17): dict(K=[20], P=[124]),
    (129, 31): dict(K=[28], P=[132]),
    (257, 33): dict(K=[36], P=[260]),
    (300, 64): dict(K=[65], P=[301]),
    (65, 530): dict(K=[531, 532], P=[68]),
    (130, 1031): dict(K=[1032], P=[131, 132]),
    (257, 1000): dict(K=[1001], P=[260]),
    (128, 2560): dict(K=[2561], P=[127]),
    (129, 2561): dict(K=[2564], P=[132]),
    (385, 1300): dict(K=[1301], P=[388]),
}
# "h+m" integers need K <= 16: the K <= 16 shapes above, and these, with
# several tiles (one chunk: 16 is less than a slice)
HM_SHAPES = [(300, 16), (129, 7)]
HM_TWINS = {(300, 16): dict(K=[13], P=[301]), (129, 7): dict(K=[8], P=[132])}


def exact_cases():
    """[(P, K, which, primary (P, K))] of the exact-integer tests: every
    listed shape and its twins, in both layouts"""
    out = []
    for table, twins in ((([s[0] for s in SHAPES]), TWINS), (HM_SHAPES, HM_TWINS)):
        for (P, K) in table:
            for which in (0, 1):
                out.append((P, K, which, (P, K)))
                if which == 0:
                    out += [(P, k, 0, (P, K)) for k in twins[(P, K)]["K"]]
                else:
                    out += [(p, K, 1, (P, K)) for p in twins[(P, K)]["P"]]
    return out


# ------------------------------------------------------------- families --
def _scale_rows(B, idx, lo, hi, rng):
    """one power of two per Gram index (exact)"""
    if idx % 3:
        return B
    e = rng.integers(lo, hi + 1, B.shape[0])
    return np.ldexp(B, e[:, None].astype(np.int32)).astype(B.dtype)


def _sig_bits(x):
    x = np.abs(x.astype(np.int64))
    low = x & -x
    return np.where(x == 0, 0, np.log2(np.maximum(x, 1)).astype(np.int64)
                    - np.log2(np.maximum(low, 1)).astype(np.int64) + 1)


@functools.lru_cache(maxsize=None)
def integers(P, K, dtype, which, idx=1):
    """Exact integers: "h+m" (|x| <= 1000, K <= 16) or "deep" (|x| <= 63,
    K <= 4000), times one power of two in [-40, 40] per Gram index when
    idx % 3 == 0.  Every product and every partial sum, in any order and
    any split, is representable: S = |B| |B|^t < 2^24."""
    rng = _rng(1, P, K, which, np.dtype(dtype).itemsize, idx)
    if K <= 16:
        Bi = rng.integers(-1000, 1001, (P, K))
        if Bi.size >= 64:
            assert np.mean(_sig_bits(Bi) > 8) >= 0.25   # the m planes carry data
    else:
        assert K <= 4000
        Bi = rng.integers(-63, 64, (P, K))
    S = np.abs(Bi) @ np.abs(Bi).T
    assert S.max() < 2 ** 24
    B = _scale_rows(Bi.astype(dtype), idx, -40, 40, rng)
    A = to_A(B, which)
    A.setflags(write=False)
    return A, which


def _fixed_mantissas(nm):
    top = 1 << (nm - 1)
    return [(1 << nm) - 1,                             # mantissa all ones
            top + 1,                                   # nextafter(1, 2)
            top + (top >> 8) + (top >> 16)]            # 1 + 2^-8 + 2^-16


@functools.lru_cache(maxsize=None)
def full_mantissa(P, K, dtype, which):
    """Random full-width mantissas (24 bits, f64: 53), signs, and one
    exponent per Gram index from [-60, 60] (products stay normal; at a
    length where a sum of K products of 2^122 would leave the f32 range the
    top of the range comes down: S < 2^127 is asserted).  Gram
    index i with i % 8 < 5 carries a fixed lane at contraction index 0:
    mantissa all ones, nextafter(1, 2), 1 + 2^-8 + 2^-16, +0.0, -0.0."""
    nm = 24 if np.dtype(dtype) == np.float32 else 53
    rng = _rng(2, P, K, which, nm)
    mant = rng.integers(1 << (nm - 1), 1 << nm, (P, K), dtype=np.int64)
    fixed = _fixed_mantissas(nm)
    zero = np.zeros((P, K), bool)
    for i in range(P):
        lane = i % 8
        if lane < 3:
            mant[i, 0] = fixed[lane]
        elif lane < 5:
            zero[i, 0] = True
    sign = np.where(rng.random((P, K)) < 0.5, -1.0, 1.0)
    sign[np.arange(P) % 8 == 3, 0] = 1.0               # +0.0
    sign[np.arange(P) % 8 == 4, 0] = -1.0              # -0.0
    top = min(60, (126 - int(np.ceil(np.log2(K)))) // 2 - 1)
    e = rng.integers(-60, top + 1, P)
    B = np.ldexp(mant.astype(np.float64), (e[:, None] - (nm - 1)).astype(np.int32))
    assert (np.abs(B) @ np.abs(B).T).max() < 2.0 ** 127
    assert np.array_equal(B.astype(dtype).astype(np.float64), B)      # nothing rounded
    B = (sign * np.where(zero, 0.0, B)).astype(dtype)
    nz = np.abs(B[B != 0]).astype(np.float64)
    assert nz.min() >= 2.0 ** -60 and nz.max() < 2.0 ** 61
    A = to_A(B, which)
    A.setflags(write=False)
    return A, which


@functools.lru_cache(maxsize=None)
def uniform(P, K, dtype, which):
    """uniform(-1, 1), the inputs of tests/test_gram_gpu.py"""
    A = to_A(_rng(3, P, K, which).uniform(-1, 1, (P, K)).astype(dtype), which)
    A.setflags(write=False)
    return A, which


TINY = (-126, -105)   # normal f32 whose l piece (below 2^-118: m too) is a bf16 subnormal


@functools.lru_cache(maxsize=None)
def tiny_huge(P, K, dtype, which, huge=(90, 100), tiny=TINY):
    """Even Gram indices scaled into [2^tiny[0], 2^tiny[1]) -- by default
    [2^-126, 2^-105]: normal f32 with subnormal bf16 pieces; one binade per
    index, every binade taken in turn, and with tiny[0] = -126 one element
    in 16 of them a true f32 subnormal -- odd ones into [2^huge[0],
    2^huge[1]), 24-bit mantissas throughout.  With huge = (90, 100) a
    huge-huge product overflows f32 (the split tile's NaN flag then hands
    the Gram to the exact tile); (40, 55) keeps every element of G finite."""
    assert np.dtype(dtype) == np.float32
    rng = _rng(4, P, K, which, huge[0], tiny[0])
    mant = rng.integers(1 << 23, 1 << 24, (P, K), dtype=np.int64).astype(np.float64)
    sign = np.where(rng.random((P, K)) < 0.5, -1.0, 1.0)
    small = np.arange(P) % 2 == 0
    e = np.where(small, tiny[0] + (np.arange(P) // 2) % (tiny[1] - tiny[0]),
                 rng.integers(huge[0], huge[1], P))
    B = sign * np.ldexp(mant, (e[:, None] - 23).astype(np.int32))
    if tiny[0] == -126:
        sub = small[:, None] & (rng.random((P, K)) < 1 / 16)
        B = np.where(sub, sign * np.ldexp(np.floor(mant / 2 ** 12), -149), B)   # 12-bit subnormals
    assert np.array_equal(B.astype(np.float32).astype(np.float64), B)
    B = B.astype(np.float32)
    a = np.abs(B.astype(np.float64))
    assert np.all(a[small] < 2.0 ** tiny[1]) and np.all(a[small] > 0)
    if tiny[0] == -126:
        assert np.any(a[small] < 2.0 ** -126) and np.any(a[small] >= 2.0 ** -126)
    else:
        assert np.all(a[small] >= 2.0 ** tiny[0])
    if P >= 2 * (tiny[1] - tiny[0]):
        assert np.unique(e[small]).size == tiny[1] - tiny[0]                    # every binade
    assert np.all(a[~small] >= 2.0 ** huge[0]) and np.all(a[~small] < 2.0 ** huge[1])
    if huge[1] <= 55:
        assert (a @ a.T).max() < 2.0 ** 127                                # nothing overflows
    A = to_A(B, which)
    A.setflags(write=False)
    return A, which


# ----------------------------------------------------------- references --
def _row_exponents(B):
    """per Gram index, the largest e with B[i] / 2^e all integers"""
    m, ex = np.frexp(B.astype(np.float64))
    mi = np.round(np.ldexp(m, 53)).astype(np.int64)
    low = np.where(mi == 0, 1 << 62, mi & -mi)
    tz = np.log2(low.astype(np.float64)).astype(np.int64)
    lowest = np.where(mi == 0, 1 << 20, ex - 53 + tz)
    e = lowest.min(axis=1)
    return np.where(e == 1 << 20, 0, e)


def integer_ref(A, which):
    """(ref, S) of an integer family, exactly: the integers are recovered
    from A (one power of two per Gram index), ref and S = |B| |B|^t formed
    in int64 (through float64 products that are exact: K max^2 < 2^53) and
    S.max() < 2^24 asserted; both returned as float64, scaled back."""
    B = rows_of(A, which)
    e = _row_exponents(B)
    Bi = np.ldexp(B.astype(np.float64), (-e[:, None]).astype(np.int32))
    assert np.array_equal(Bi, np.round(Bi))
    assert B.shape[1] * max(1.0, np.abs(Bi).max()) ** 2 < 2.0 ** 53
    ref = (Bi @ Bi.T).astype(np.int64)
    S = (np.abs(Bi) @ np.abs(Bi).T).astype(np.int64)
    assert S.max(initial=0) < 2 ** 24
    sc = (e[:, None] + e[None, :]).astype(np.int32)
    return np.ldexp(ref.astype(np.float64), sc), np.ldexp(S.astype(np.float64), sc)


def exact_ref(A, which):
    """the result a correct kernel owes on an integer family, in A's type"""
    ref, _ = integer_ref(A, which)
    out = ref.astype(A.dtype)
    assert np.array_equal(out.astype(np.float64), ref)
    return out


def normalised_error(G, A, which, integer=False):
    """|G - ref| / S element-wise, S = |B| |B|^t.  ref and S in float64
    (int64 for the integer families; long double for an f64 A, whose own
    rounding would otherwise be the kernel's size).  Elements with S == 0
    must be exactly 0 in G."""
    B = rows_of(A, which)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if integer:
            ref, S = integer_ref(A, which)
        else:
            wide = np.longdouble if A.dtype == np.float64 else np.float64
            Bw = np.ascontiguousarray(B).astype(wide)
            ref, S = Bw @ Bw.T, np.abs(Bw) @ np.abs(Bw).T
        assert G.shape == ref.shape
        zero = S == 0
        assert np.all(G[zero] == 0)
        err = np.abs(G.astype(ref.dtype) - ref) / np.where(zero, 1, S)
    return np.where(zero, 0.0, err).astype(np.float64)


def chain_f32(A, which):
    """the plain f32 reference of the same operation: G <- fl(G + fl(a_k
    a_k^t)), k ascending, in numpy f32"""
    B = np.ascontiguousarray(rows_of(A, which).T, dtype=np.float32)   # K x P
    P = B.shape[1]
    G = np.zeros((P, P), np.float32)
    tmp = np.empty_like(G)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for a in B:
            np.multiply.outer(a, a, out=tmp)
            G += tmp
    return G


def sample_indices(P, K, work=4e8):
    """Gram indices of the sub-block an element-wise check looks at when P
    x P x K is too much for a numpy reference: evenly spread, both ends
    included; all of them when they fit"""
    n = int(min(P, max(32, np.sqrt(work / max(K, 1)))))
    return np.arange(P) if n >= P else np.unique(np.round(np.linspace(0, P - 1, n)).astype(int))


def sub_block(G, A, which, idx):
    """(G, A) restricted to the Gram indices idx: the Gram of a subset of
    indices is the sub-block"""
    return G[np.ix_(idx, idx)], (A[:, idx] if which == 0 else A[idx])


# ---------------------------------------------------- the split in numpy --
def split_model(A, which):
    """k_gram_b in numpy for a short contraction (one 16-k MFMA step): the
    six piece products, each exact in f32, added in the kernel's order (hh;
    hm, mh, mm; hl, lh -- each over k ascending) by sequential f32 adds"""
    from test_gram_split_cpu import split3
    B = rows_of(A, which).astype(np.float32)
    assert B.shape[1] <= 16
    h, m, l, _ = split3(B)
    G = np.zeros((B.shape[0],) * 2, np.float32)
    with np.errstate(under="ignore"):
        for x, y in ((h, h), (h, m), (m, h), (m, m), (h, l), (l, h)):
            for k in range(B.shape[1]):
                G += np.multiply.outer(x[:, k], y[:, k])
    return G


# The split tile against the plain f32 chain: the largest measured ratio of
# their largest normalised errors (2.9, at K = 37; 0.06-0.14 at K = 1300 and
# 20000), rounded up to the next power of two
# (tests/test_gram_exact_gpu.py test_working_length_split has the figures)
SPLIT_MARGIN = 4


def split_bar(chain_max):
    return chain_max * SPLIT_MARGIN + 2.0 ** -21


def length_bound(P, K, dtype, split=True):
    """derived worst case of the exact tiles and of f64 at length: one
    rounding per product and per addition, and the pass over the chunks"""
    return 2 * (K + plan(P, K, dtype, split)["nchunk"]) * unit(dtype)


def split_bound(K):
    """derived, for K <= 2: the dropped pieces (2^-21, test_gram_split_cpu)
    plus 6 K accumulations, each allowed a full ulp (2 u)"""
    return 2.0 ** -21 + 12 * K * 2.0 ** -24
