"""GPU: the Gram tiles (csrc/pfdr_gram.hip) element by element, against
exact integer results and float64 / long double references, on every tile,
layout, load path and gram_block branch (cases: tests/gram_cases.py, checked
on the CPU by tests/test_gram_cases_cpu.py).

Which test reaches which instantiation (TN: which = 0, NT: which = 1; the
16-byte path "v" when ld = A.shape[0] is a multiple of 16 / itemsize and the
device pointer is 16-byte aligned, else the scalar path "s"):

  k_gram_b<TN|NT, 16, true|false>   test_exact_integers[f32], test_zero_length,
                                    test_piece_algebra_split, test_working_length_split,
                                    test_tiny_against_huge_split[edge], test_tiny_short,
                                    test_device_entry (v), test_device_misaligned (s)
  k_gram_v<float, TN|NT>            test_exact_integers_exact_tile, test_piece_algebra_exact_tile,
                                    test_working_length_exact_tile, test_tiny_against_huge_exact_tile
                                    (child process, PFDR_GRAM_SPLIT=0); in process through the
                                    flag: test_fallback_at_size, test_tiny_against_huge_split[issue, finite],
                                    test_single_small_element_is_flagged
  k_gram<float, TN|NT>              the same tests, on their scalar-ld cases
  k_gram_v<double, TN|NT>           test_exact_integers[f64], test_piece_algebra_f64,
  k_gram<double, TN|NT>             test_working_length_f64 (vector only), test_device_entry,
                                    test_device_misaligned (scalar)

Each of them runs with several tiles and several chunks in
test_exact_integers / test_exact_integers_exact_tile ((130, 1031), (257,
1000), (129, 2561), (385, 1300) and their twins of the other ld parity;
tests/test_gram_cases_cpu.py asserts that through the chunk plan).

Bounds (u = 2^-24 for f32, 2^-53 for f64; errors are |G - ref| / S with S =
|B| |B|^t, element-wise):
  integers                      np.array_equal: S < 2^24, so every partial sum
                                in any order and any split is representable
  K <= 2, split tile            2^-21 + 12 K 2^-24: the dropped pieces (ml, lm,
                                ll: tests/test_gram_split_cpu.py) plus 6 K
                                accumulations of at most one ulp each
  exact tiles and f64           2 K u for K <= 2, 2 (K + nchunk) u at length:
                                one rounding per product and per addition, and
                                the second pass over the chunks
  split tile at length          chain_max * SPLIT_MARGIN + 2^-21, chain_max the
                                error of the plain f32 chain (gram_cases.chain_f32)
                                on the same input; see test_working_length
All derived, none read off the kernel -- but gram_cases.SPLIT_MARGIN, which
is the measured ratio rounded up to a power of two, as its test says."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gram_cases as gc
from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F32, F64 = np.float32, np.float64

# -------------------------------------------------------------- cases --
EXACT = gc.exact_cases()
EXACT_IDS = ["%s-%dx%d-w%d" % ("hm" if K <= 16 else "deep", P, K, w) for P, K, w, _ in EXACT]

# K in {1, 2}; which = 0 has ld = K, so its 16-byte parity is a 4-long
# contraction whose last rows are zero (they add exact zeros); which = 1
# has ld = P: 128, 300 vector, 127, 301 scalar
SHORT = [(P, K, 0, pad) for P in (128, 300) for K in (1, 2) for pad in (0, 4)] + \
        [(P, K, 1, 0) for P in (128, 127, 300, 301) for K in (1, 2)]
SHORT_IDS = ["%dx%d-w%d%s" % (P, K, w, "-ld4" if pad else "") for P, K, w, pad in SHORT]


def _short(P, K, dt, which, pad):
    A, w = gc.full_mantissa(P, K, dt, which)
    if pad:
        A = np.concatenate([A, np.zeros((pad - K, P), dt)])
    return A, w


WORK = [(P, K, w, fam) for (P, K) in ((200, 1300), (96, 20000)) for w in (0, 1)
        for fam in ("uniform", "full_mantissa")]
WORK_IDS = ["%s-%dx%d-w%d" % (fam, P, K, w) for P, K, w, fam in WORK]

# (huge, tiny) ranges.  "issue": the family as first stated; its huge-huge
# products overflow f32, the split tile flags a NaN and the exact tile
# answers.  "finite": huge in [2^40, 2^55) keeps all of G finite; the split
# tile's staging pass flags the elements below 2^-109, which it cannot split
# exactly, and the exact tile answers again.  "edge": the binades from 2^-109
# up, which the split tile keeps: their l pieces are bf16 subnormals (l <=
# 2^-16 x < 2^-126 up to 2^-110, and often beyond), split without loss and,
# as these cases measure, kept by the matrix cores.
TINY_RANGES = {"issue": ((90, 100), gc.TINY), "finite": ((40, 55), gc.TINY),
               "edge": ((40, 55), (-109, -103))}
TINY = [(P, K, w, name) for (P, K) in ((129, 31), (130, 1031)) for w in (0, 1)
        for name in TINY_RANGES]
TINY_IDS = ["%dx%d-w%d-%s" % c for c in TINY]


def _tiny(P, K, w, name):
    huge, tiny = TINY_RANGES[name]
    return gc.tiny_huge(P, K, F32, w, huge, tiny)


def _child_inputs():
    out = {}
    for n, (P, K, w, _) in enumerate(EXACT):
        out["int-" + EXACT_IDS[n]] = gc.integers(P, K, F32, w, n)
    for c, cid in zip(SHORT, SHORT_IDS):
        out["short-" + cid] = _short(c[0], c[1], F32, c[2], c[3])
    for (P, K, w, fam), cid in zip(WORK, WORK_IDS):
        out["work-" + cid] = getattr(gc, fam)(P, K, F32, w)
    for c, cid in zip(TINY, TINY_IDS):
        out["tiny-" + cid] = _tiny(*c)
    return out


@pytest.fixture(scope="module")
def exact_tile(gpu_lib, tmp_path_factory):
    """every f32 case on the exact-f32 tiles: one fresh child process with
    PFDR_GRAM_SPLIT=0 (gram() reads it once per process)"""
    d = tmp_path_factory.mktemp("gram_child")
    src, dst = str(d / "in.npz"), str(d / "out.npz")
    cases = _child_inputs()
    arrays = {}
    for name, (A, w) in cases.items():
        arrays["A." + name] = A
        arrays["w." + name] = np.int32(w)
    np.savez(src, **arrays)
    env = dict(os.environ, PFDR_GRAM_SPLIT="0")
    r = subprocess.run([sys.executable, "tests/gram_child.py", src, dst], env=env, cwd=ROOT,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, "gram_child.py exit %d\n%s" % (r.returncode, r.stderr[-2000:])
    with np.load(dst) as z:
        return {name: z["G." + name] for name in cases}


def _gram(A, which):
    G, _ = pfdr.gram(A, which)
    assert G.shape == (gc.rows_of(A, which).shape[0],) * 2
    return G


# ------------------------------------------------- 1, 2: exact integers --
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", range(len(EXACT)), ids=EXACT_IDS)
def test_exact_integers(gpu_lib, n, dt):
    """default process: f32 on k_gram_b, f64 on k_gram_v / k_gram"""
    P, K, w, _ = EXACT[n]
    A, w = gc.integers(P, K, dt, w, n)
    assert np.array_equal(_gram(A, w), gc.exact_ref(A, w))


@pytest.mark.parametrize("n", range(len(EXACT)), ids=EXACT_IDS)
def test_exact_integers_exact_tile(exact_tile, n):
    """the same f32 cases on k_gram_v<float> / k_gram<float>"""
    P, K, w, _ = EXACT[n]
    A, w = gc.integers(P, K, F32, w, n)
    assert np.array_equal(exact_tile["int-" + EXACT_IDS[n]], gc.exact_ref(A, w))


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("P", [1, 127, 300])
def test_zero_length(gpu_lib, P, dt):
    """K = 0 (M = 0, which = 0): G is all zeros"""
    G = _gram(np.zeros((0, P), dt), 0)
    assert G.dtype == dt and np.array_equal(G, np.zeros((P, P), dt))


# ------------------------------------------------ 3: fallback at size --
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("shape", [(257, 1000), (257, 1001), (260, 1000), (130, 1031),
                                   (130, 1032), (131, 1031), (132, 1031)])
def test_fallback_at_size(gpu_lib, shape, which):
    """one infinite entry on several tiles and chunks: the NaN flag sends
    the Gram to the exact-f32 tile (vector or scalar by ld).  The entry's
    row and column are its signed infinities, every other element the exact
    integer (the column that meets the infinity holds no zero: inf x 0)"""
    P, K = shape
    pl = gc.plan(P, K, F32)
    assert pl["tiles"] > 1 and pl["nchunk"] > 1
    A, _ = gc.integers(P, K, F32, which, 1)
    B = gc.rows_of(A, which).copy()
    r, c = P - 2, K - 3                       # last tile, last chunk
    B[B[:, c] == 0, c] = 1
    want_rc = np.sign(B[:, c]).astype(F32) * F32(np.inf)
    B[r, c] = np.inf
    want_rc[r] = np.inf
    A = gc.to_A(B, which)
    G = _gram(A, which)
    assert np.array_equal(G[r], want_rc) and np.array_equal(G[:, r], want_rc)
    keep = np.arange(P) != r
    A_keep = A[:, keep] if which == 0 else A[keep]
    assert np.array_equal(G[np.ix_(keep, keep)], gc.exact_ref(A_keep, which))


# ------------------------------------------------- 4: piece algebra --
def _check_short(G, A, w, K, bound):
    err = gc.normalised_error(G, A, w)
    print("K=%d max %.2f x u (bound %.2f x u)" % (K, err.max() / gc.unit(A.dtype),
                                                 bound / gc.unit(A.dtype)))
    assert np.array_equal(G, G.T)
    assert err.max() <= bound


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_piece_algebra_split(gpu_lib, case):
    """K = 1: G is an outer product, each element one six-piece product.  A
    dropped or misrouted l plane costs 2^-18 to 2^-16 of a product"""
    P, K, w, pad = case
    A, w = _short(P, K, F32, w, pad)
    _check_short(_gram(A, w), A, w, K, gc.split_bound(K))


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_piece_algebra_exact_tile(exact_tile, case):
    P, K, w, pad = case
    A, w = _short(P, K, F32, w, pad)
    _check_short(exact_tile["short-" + SHORT_IDS[SHORT.index(case)]], A, w, K, 2 * K * 2.0 ** -24)


@pytest.mark.parametrize("case", SHORT, ids=SHORT_IDS)
def test_piece_algebra_f64(gpu_lib, case):
    P, K, w, pad = case
    A, w = _short(P, K, F64, w, pad)
    _check_short(_gram(A, w), A, w, K, 2 * K * 2.0 ** -53)


# -------------------------------------------- 5: working length --
@pytest.fixture(scope="module")
def chain_max():
    """max normalised error of the plain f32 chain, once per input"""
    memo = {}

    def get(name, A, w, mask=None):
        if name not in memo:
            err = gc.normalised_error(gc.chain_f32(A, w), A, w)
            memo[name] = float(err.max() if mask is None else err[mask].max())
        return memo[name]
    return get


@pytest.mark.parametrize("case", WORK, ids=WORK_IDS)
def test_working_length_split(gpu_lib, chain_max, case):
    """The split tile has no useful derived bound at this length (6 K
    accumulations of one ulp each), so it is measured against the plain f32
    chain on the same input: bar = chain_max * SPLIT_MARGIN + 2^-21.

    Measured on an MI355X, largest normalised error in units of u = 2^-24
    (kernel / chain = ratio), uniform and full-mantissa inputs, both layouts:
      (200, 1300)    3.2-3.7 u  / 26.5-30.3 u  = 0.11-0.14
      (96, 20000)    7.8-11.7 u / 88-125 u     = 0.06-0.13
    (the exact-f32 tile on the same inputs: 3.5-4.3 u and 7.2-8.5 u: the MFMA
    chains are blocked sums, far shorter than the plain chain.)  On the short
    contractions of tests/test_gram_gpu.py the six-piece products weigh more
    and the ratio is above one: 2.9 on (100, 37) A A^t (K = 37: 10.4 u
    against 3.6 u), 1.4 on its A^t A (K = 100), 1.2 on (64, 3000) and (96,
    4096) A^t A, below 0.6 from K = 256 up.  gram_cases.SPLIT_MARGIN is the
    largest of them, 2.9, rounded up to the next power of two: 4 (never
    above 16: a six-piece product may err 8 u where an f32 product rounds
    at u / 2)."""
    P, K, w, fam = case
    A, w = getattr(gc, fam)(P, K, F32, w)
    kmax = gc.normalised_error(_gram(A, w), A, w).max()
    cmax = chain_max(WORK_IDS[WORK.index(case)], A, w)
    print("split %s: kernel %.2f u, chain %.2f u, ratio %.3f" % (
        WORK_IDS[WORK.index(case)], kmax * 2 ** 24, cmax * 2 ** 24, kmax / cmax))
    assert kmax <= gc.split_bar(cmax)


@pytest.mark.parametrize("case", WORK, ids=WORK_IDS)
def test_working_length_exact_tile(exact_tile, chain_max, case):
    P, K, w, fam = case
    A, w = getattr(gc, fam)(P, K, F32, w)
    name = WORK_IDS[WORK.index(case)]
    kmax = gc.normalised_error(exact_tile["work-" + name], A, w).max()
    bound = gc.length_bound(P, K, F32, split=False)
    print("exact tile %s: kernel %.2f u, chain %.2f u, bound %.0f u" % (
        name, kmax * 2 ** 24, chain_max(name, A, w) * 2 ** 24, bound * 2 ** 24))
    assert kmax <= bound


@pytest.mark.parametrize("case", WORK, ids=WORK_IDS)
def test_working_length_f64(gpu_lib, case):
    P, K, w, fam = case
    A, w = getattr(gc, fam)(P, K, F64, w)
    kmax = gc.normalised_error(_gram(A, w), A, w).max()
    bound = gc.length_bound(P, K, F64)
    print("f64 %s: kernel %.2f u, bound %.0f u" % (WORK_IDS[WORK.index(case)], kmax * 2 ** 53,
                                                  bound * 2 ** 53))
    assert kmax <= bound


# -------------------------------------------- 6: tiny against huge --
def _tiny_check(G, A, w, bar):
    """elements whose S is inside the normal range are held to the bar; S
    below half the smallest subnormal (tiny x tiny) is an exact zero;
    elements past the f32 range (huge x huge of the "issue" family)
    are the exact tile's overflow and not looked at"""
    B = gc.rows_of(A, w).astype(np.float64)
    S = np.abs(B) @ np.abs(B).T
    P = S.shape[0]
    tiny = np.arange(P) % 2 == 0
    held = (S >= 2.0 ** -120) & (S < 2.0 ** 127)
    assert np.all(held[np.ix_(tiny, ~tiny)]) and np.all(held[np.ix_(~tiny, tiny)])
    assert np.all(G[S < 2.0 ** -150] == 0)
    err = gc.normalised_error(G, A, w)
    worst = err[held].max()
    assert worst <= bar, "%.3g u against %.3g u" % (worst * 2 ** 24, bar * 2 ** 24)
    return held, worst


@pytest.mark.parametrize("case", TINY, ids=TINY_IDS)
def test_tiny_against_huge_split(gpu_lib, chain_max, case):
    """A normal f32 below 2^-110 has a subnormal l piece (below 2^-118 the m
    piece too).  Measured on an MI355X: v_mfma_f32_32x32x16_bf16 KEEPS
    subnormal bf16 inputs ("edge": 5.7-6.2 u at K = 31, 2.8 u at K = 1031;
    test_tiny_short holds the same binades to the K <= 2 bound, which one
    flushed l would miss by 2^-17).  But the split itself loses the bits of
    an element that lie below 2^-133, the last bf16 subnormal: before the
    staging pass flagged elements below 2^-109, the "finite" cases erred
    by 2^-134 / |x| per product -- 46 u in the 2^-118 binade, 15,000 u in
    the 2^-126 one at K = 31, as the numpy model of the split does.  Now
    such an element sends the Gram to the exact-f32 tile, which keeps f32
    subnormals ("issue", "finite": 2-6 u)."""
    P, K, w, name = case
    A, w = _tiny(*case)
    G = _gram(A, w)
    B = gc.rows_of(A, w).astype(np.float64)
    S = np.abs(B) @ np.abs(B).T
    held = (S >= 2.0 ** -120) & (S < 2.0 ** 127)
    cid = TINY_IDS[TINY.index(case)]
    cmax = chain_max("tiny-" + cid, A, w, held)
    if name != "issue":
        assert np.all(np.isfinite(G))
    print("tiny %s: chain %.2f u" % (cid, cmax * 2 ** 24))
    _, worst = _tiny_check(G, A, w, gc.split_bar(cmax))
    print("tiny %s: kernel %.2f u" % (cid, worst * 2 ** 24))


@pytest.mark.parametrize("case", TINY, ids=TINY_IDS)
def test_tiny_against_huge_exact_tile(exact_tile, case):
    """the exact-f32 tile keeps f32 subnormals: what the fallback relies on"""
    P, K, w, name = case
    A, w = _tiny(*case)
    cid = TINY_IDS[TINY.index(case)]
    _, worst = _tiny_check(exact_tile["tiny-" + cid], A, w, gc.length_bound(P, K, F32, split=False))
    print("tiny %s exact tile: %.2f u" % (cid, worst * 2 ** 24))


TINY_SHORT = [(P, K, w) for P in (128, 129) for K in (1, 2) for w in (0, 1)]


@pytest.mark.parametrize("case", TINY_SHORT, ids=["%dx%d-w%d" % c for c in TINY_SHORT])
def test_tiny_short(gpu_lib, case):
    """the "edge" binades at K <= 2, on the split tile: each element of the
    tiny-huge blocks is one or two six-piece products with a subnormal l,
    held to the K <= 2 bound (a flushed l costs up to 2^-17 of a product)"""
    P, K, w = case
    A, w = gc.tiny_huge(P, K, F32, w, (40, 55), (-109, -103))
    G = _gram(A, w)
    assert np.all(np.isfinite(G)) and np.array_equal(G, G.T)
    _, worst = _tiny_check(G, A, w, gc.split_bound(K))
    print("tiny short %dx%d-w%d: %.2f u (bound %.0f u)" % (P, K, w, worst * 2 ** 24,
                                                          gc.split_bound(K) * 2 ** 24))


SINGLE = [(P, K, w, pos) for (P, K) in ((129, 31), (130, 1031)) for w in (0, 1)
          for pos in ("first", "last", "second-tile")]


@pytest.mark.parametrize("case", SINGLE, ids=["%dx%d-w%d-%s" % c for c in SINGLE])
def test_single_small_element_is_flagged(gpu_lib, case):
    """one element of the 2^-126 binade alone in its row (so that it is the
    whole of its products), anywhere in A -- first row and k, last row and k
    (the tails of the last tile and chunk), a row of the second tile in a
    middle chunk: only the diagonal blocks look for it, and between them
    they must see every element.  Unflagged, the split tile loses 2^-8 of
    each of its products; the exact tile answers within its derived bound."""
    P, K, w, pos = case
    A, w = gc.tiny_huge(P, K, F32, w, (40, 55), (-109, -103))
    B = gc.rows_of(A, w).copy()
    r, k = {"first": (0, 0), "last": ((P - 1) // 2 * 2, K - 1), "second-tile": (128, K // 2)}[pos]
    assert r % 2 == 0 and r < P
    x = np.ldexp(np.float32(B[r, k]), -126 - int(np.floor(np.log2(abs(B[r, k])))))
    assert 2.0 ** -126 <= abs(x) < 2.0 ** -125
    B[r] = 0
    B[r, k] = x
    A = gc.to_A(B, w)
    _, worst = _tiny_check(_gram(A, w), A, w, gc.length_bound(P, K, F32))
    print("single small element %s: %.2f u" % (pos, worst * 2 ** 24))


# -------------------------------------------- 7: device entry, alignment --
def _device_case(dt, which):
    """(257, 1000) "deep" integers; which = 1 on P = 260, so that ld = M is
    a multiple of 4 in both layouts"""
    P, K = (257, 1000) if which == 0 else (260, 1000)
    A, w = gc.integers(P, K, dt, which, 1)
    assert A.shape[0] % 4 == 0 and gc.plan(P, K, dt)["nchunk"] >= 8
    return A, w


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", [0, 1])
def test_device_entry(gpu_lib, which, dt):
    """gram(device=True) on a torch tensor: the host call's bytes"""
    import torch
    A, w = _device_case(dt, which)
    host = _gram(A, w)
    M, N = A.shape
    T = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()      # (N, M): column-major M x N
    assert T.shape == (N, M) and T.data_ptr() % 16 == 0
    G, _ = pfdr.gram(T, w, device=True)
    torch.cuda.synchronize()
    G = G.cpu().numpy()
    assert G.tobytes() == host.tobytes()
    assert np.array_equal(G, gc.exact_ref(A, w))


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("which", [0, 1])
def test_device_misaligned(gpu_lib, which, dt):
    """the matrix one element into a larger buffer, ld a multiple of 4:
    gram() tests the pointer ((uintptr_t)A % 16), finds it unaligned and
    takes the scalar tile -- no 16-byte load is issued.  Result: exact."""
    import torch
    A, w = _device_case(dt, which)
    M, N = A.shape
    buf = torch.zeros(M * N + 8, dtype=torch.float32 if dt == F32 else torch.float64,
                      device="cuda")
    assert buf.data_ptr() % 16 == 0
    T = buf[1:1 + M * N].view(N, M)
    T.copy_(torch.from_numpy(np.ascontiguousarray(A.T)))
    assert T.data_ptr() % 16 == A.dtype.itemsize and T.is_contiguous()
    G, _ = pfdr.gram(T, w, device=True)
    torch.cuda.synchronize()
    assert np.array_equal(G.cpu().numpy(), gc.exact_ref(A, w))
