"""CPU: the cases of tests/test_gram_exact_gpu.py are what they claim to be
(tests/gram_cases.py): every integer case is exactly representable, every
listed shape runs the tiles, chunks and gram_block branch its comment names,
and the numpy model of the split tile passes the K <= 2 bound on its own."""
import numpy as np
import pytest

import gram_cases as gc


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_integer_cases_are_exactly_representable(dt):
    scaled = 0
    for n, (P, K, which, _) in enumerate(gc.exact_cases()):
        A, w = gc.integers(P, K, dt, which, n)
        assert A.shape == ((K, P) if which == 0 else (P, K)) and A.dtype == dt
        ref, S = gc.integer_ref(A, w)                    # asserts S.max() < 2^24
        B = gc.rows_of(A, w).astype(np.float64)
        assert np.array_equal(ref, B @ B.T)
        assert np.array_equal(gc.exact_ref(A, w).astype(np.float64), ref)
        assert np.all(gc.normalised_error(ref.astype(dt), A, w, integer=True) == 0)
        scaled += n % 3 == 0
    assert 3 * scaled >= len(gc.exact_cases())           # a third carry a power of two


def test_integer_precondition_catches_a_bad_case():
    B = np.full((4, 17), 999.0, np.float32)              # 17 x 999^2 >= 2^24
    with pytest.raises(AssertionError):
        gc.integer_ref(B, 1)


@pytest.mark.parametrize("shape,f32,f64", gc.SHAPES)
def test_listed_shapes_exercise_what_they_claim(shape, f32, f64):
    P, K = shape
    for dt, want in ((np.float32, f32), (np.float64, f64)):
        for split in (True, False):                      # the chunk target does not bind here
            got = gc.plan(P, K, dt, split)
            for key, val in want.items():
                assert got[key] == val, (shape, dt.__name__, key, got)
    # the twins keep the shape's character: as many tiles, one chunk or many
    base = gc.plan(P, K, np.float32)
    for k in gc.TWINS[shape]["K"]:
        t = gc.plan(P, k, np.float32)
        assert t["tiles"] == base["tiles"] and (t["nchunk"] > 1) == (base["nchunk"] > 1)
    for p in gc.TWINS[shape]["P"]:
        t = gc.plan(p, K, np.float32)
        assert (t["tiles"] > 1) == (base["tiles"] > 1) and (t["nchunk"] > 1) == (base["nchunk"] > 1)


def test_every_load_path_meets_tiles_and_chunks():
    """each of the two load paths runs, in each layout and type, on a case
    with more than one tile and more than one chunk"""
    for dt in (np.float32, np.float64):
        for which in (0, 1):
            seen = set()
            for P, K, w, _ in gc.exact_cases():
                pl = gc.plan(P, K, dt)
                if w == which and pl["tiles"] > 1 and pl["nchunk"] > 1:
                    M = K if which == 0 else P
                    seen.add(M % (16 // np.dtype(dt).itemsize) == 0)
            assert seen == {True, False}, (dt.__name__, which)


def test_plan_of_the_frobenius_shapes():
    """tests/test_gram_gpu.py: the chunk counts its comments name"""
    assert gc.plan(2048, 20000, np.float32)["nchunk"] == 32
    assert gc.plan(2048, 20000, np.float32)["kchunk"] == 640
    assert gc.plan(2048, 20000, np.float32)["last"] == 160
    assert gc.plan(96, 20000, np.float32)["nchunk"] == 157
    assert gc.plan(3000, 64, np.float32)["tiles"] == 300
    assert gc.plan(4096, 96, np.float32)["tiles"] == 528
    assert gc.plan(0 + 1, 0, np.float32)["nchunk"] == 1


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("P", [128, 300])
def test_split_model_inside_the_short_bound(P, K):
    """the reference alone passes the bar of the GPU test (it sits at 3.8 x 2^-24
    for K = 1 and 6.2 x 2^-24 for K = 2, of 20 and 32 allowed), and an l plane left out does not"""
    from test_gram_split_cpu import split3
    worst = 0.0
    for which in (0, 1):
        A, w = gc.full_mantissa(P, K, np.float32, which)
        G = gc.split_model(A, w)
        err = gc.normalised_error(G, A, w).max()
        worst = max(worst, err)
        assert err <= gc.split_bound(K)
        # without hl + lh: about 2^-16 per product, far outside
        B = gc.rows_of(A, w).astype(np.float32)
        h, m, l, _ = split3(B)
        hl = sum(np.multiply.outer(h[:, k], l[:, k]).astype(np.float64) for k in range(K))
        assert gc.normalised_error((G - (hl + hl.T)).astype(np.float32), A, w).max() > gc.split_bound(K)
    print("split model P=%d K=%d: %.2f x 2^-24" % (P, K, worst * 2 ** 24))


def test_families_hold_their_preconditions():
    for which in (0, 1):
        for dt in (np.float32, np.float64):
            A, _ = gc.full_mantissa(300, 2, dt, which)
            B = gc.rows_of(A, which)
            nm = 24 if dt == np.float32 else 53
            m = [abs(np.frexp(B[i, 0])[0]) * 2 for i in range(3)]    # mantissas in [1, 2)
            assert m[0] == 2 - 2.0 ** (1 - nm) and m[1] == np.nextafter(dt(1), dt(2))
            assert m[2] == 1 + 2.0 ** -8 + 2.0 ** -16
            assert B[3, 0] == 0 and not np.signbit(B[3, 0]) and np.signbit(B[4, 0])
        for huge, tiny in (((90, 100), gc.TINY), ((40, 55), gc.TINY), ((40, 55), (-109, -103))):
            A, _ = gc.tiny_huge(129, 31, np.float32, which, huge, tiny)   # asserts its own ranges
            assert A.shape == ((31, 129) if which == 0 else (129, 31))


def test_chain_f32_is_the_sequential_sum():
    A, w = gc.uniform(5, 40, np.float32, 1)
    G = gc.chain_f32(A, w)
    s = np.float32(0)
    for k in range(40):
        s = np.float32(s + np.float32(A[1, k] * A[3, k]))
    assert G[1, 3] == s and np.array_equal(G, G.T)
    idx = gc.sample_indices(2048, 20000)
    assert idx[0] == 0 and idx[-1] == 2047 and 32 <= idx.size <= 2048
    assert gc.sample_indices(96, 20000).size == 96


def test_split_is_exact_down_to_2_pow_minus_110_only():
    """bf16 subnormals end at 2^-133: an element from 2^-110 up splits into
    its three pieces without loss (l a bf16 subnormal up to 2^-110 and
    beyond), one below loses the bits under 2^-133 -- why the split tile
    hands a Gram with a non-zero element below 2^-109 to the exact tile"""
    from test_gram_split_cpu import split3
    rng = np.random.default_rng(8)
    mant = rng.integers(1 << 23, 1 << 24, 4000).astype(np.float64)
    for e, exact in ((-110, True), (-109, True), (-111, False), (-126, False)):
        x = np.ldexp(mant, e - 23).astype(np.float32)
        h, m, l, r2 = split3(x)
        same = np.array_equal(h.astype(np.float64) + m + l, x.astype(np.float64))
        assert same == exact, e
        if exact and e == -110:
            assert np.mean(np.abs(l[l != 0]) < 2.0 ** -126) > 0.9    # bf16 subnormals
    # and the model of the tile stays inside the K <= 2 bound on those binades
    for K in (1, 2):
        A, w = gc.tiny_huge(128, K, np.float32, 1, (40, 55), (-109, -103))
        err = gc.normalised_error(gc.split_model(A, w), A, w)
        small = np.arange(128) % 2 == 0
        assert err[np.ix_(small, ~small)].max() <= gc.split_bound(K)
