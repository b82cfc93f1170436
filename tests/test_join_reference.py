"""The yardstick of the join tests (tests/join_ref.py) against the definition of include/m4ri_hip_join.h, on the CPU: a loop over all
NA * NB pairs on pools of at most 200 rows, sorted by (key, ia, ib); the weights against a bit-by-bit count.  No library, no device."""
import numpy as np
import pytest

import gf2util as g
import join_ref as jr
from lf2_ref import keys


def set_keys(words, c0, b, k):
    """bits [c0, c0 + b) of row i <- k[i], bit by bit"""
    for j in range(b):
        w, s = (c0 + j) >> 6, np.uint64((c0 + j) & 63)
        bit = (np.asarray(k).astype(np.uint64) >> np.uint64(j)) & np.uint64(1)
        words[:, w] = (words[:, w] & ~(np.uint64(1) << s)) | (bit << s)
    return words


def by_definition(A, B, ncols, c0, b, wc0, wc1):
    """every (i, j) with equal windows, ordered by (key, i, j); D and its weights from the bits"""
    to_bits = lambda w: g.words_to_bits(w, ncols) if len(w) else np.zeros((0, ncols), dtype=np.uint8)  # noqa: E731
    bits_a, bits_b = to_bits(A), to_bits(B)
    key = lambda bits, i: sum(int(bits[i, c0 + j]) << j for j in range(b))  # noqa: E731
    found = sorted((key(bits_a, i), i, j) for i in range(len(A)) for j in range(len(B)) if key(bits_a, i) == key(bits_b, j))
    ia = np.array([i for _, i, _ in found], dtype=np.int32)
    ib = np.array([j for _, _, j in found], dtype=np.int32)
    dbits = bits_a[ia] ^ bits_b[ib] if found else np.zeros((0, ncols), dtype=np.uint8)
    wt = dbits[:, wc0:wc1].sum(axis=1).astype(np.int32)
    return len(found), ia, ib, dbits, wt


def check(A, B, ncols, c0, b, wc0, wc1):
    count, ia, ib, dbits, wt = by_definition(A, B, ncols, c0, b, wc0, wc1)
    got = jr.join(A, B, ncols, c0, b, wc0, wc1)
    assert got.count == count == len(got.ia) == jr.pair_count(keys(A, c0, b), keys(B, c0, b))
    assert np.array_equal(got.ia, ia) and np.array_equal(got.ib, ib)
    assert np.array_equal(g.words_to_bits(got.D, ncols), dbits) if count else got.D.shape[0] == 0
    assert np.array_equal(got.wt, wt)
    if count and b:
        assert not keys(got.D, c0, b).any()            # the window of D is zero
    for limit in (0, 1, count // 2, count, count + 5):
        part = jr.join(A, B, ncols, c0, b, wc0, wc1, limit=limit)
        n = min(limit, count)
        assert part.count == count and np.array_equal(part.ia, ia[:n]) and np.array_equal(part.ib, ib[:n])
        assert np.array_equal(part.wt, wt[:n])
    return got


CASES = [(130, 60, 9, 3, 127), (200, 0, 4, 64, 128), (64, 37, 5, 0, 64), (65, 64, 1, 10, 11), (256, 100, 30, 70, 200), (130, 121, 9, 0, 130)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-b%d" % c[:3])
def test_random_pools_against_the_definition(case):
    ncols, c0, b, wc0, wc1 = case
    rng = np.random.default_rng(ncols + b)
    for NA, NB in ((0, 5), (5, 0), (1, 1), (37, 200), (200, 41), (120, 120)):
        values = rng.integers(0, 1 << b, 12)
        A = set_keys(g.random_words(NA, ncols, 1 + NA), c0, b, values[rng.integers(0, 12, NA)])
        B = set_keys(g.random_words(NB, ncols, 2 + NB), c0, b, values[rng.integers(0, 12, NB)])
        got = check(A, B, ncols, c0, b, wc0, wc1)
        if NA == 0 or NB == 0:
            assert got.count == 0


def test_empty_classes_on_either_side_and_duplicates():
    ncols, c0, b = 130, 50, 20
    # keys 1, 2 in A only; 7, 9 in B only; 3, 5 in both, several rows each
    ka = np.array([3, 1, 5, 3, 2, 5, 5, 1, 3])
    kb = np.array([9, 5, 3, 7, 3, 9, 5, 7])
    A = set_keys(g.random_words(len(ka), ncols, 3), c0, b, ka)
    B = set_keys(g.random_words(len(kb), ncols, 4), c0, b, kb)
    B[4] = A[0]                                   # a repeated row: a zero row in D
    got = check(A, B, ncols, c0, b, 0, ncols)
    assert got.count == 3 * 2 + 3 * 2
    # the order is (key, ia, ib)
    assert list(zip(got.ia, got.ib))[:6] == [(0, 2), (0, 4), (3, 2), (3, 4), (8, 2), (8, 4)]
    assert list(zip(got.ia, got.ib))[6:] == [(2, 1), (2, 6), (5, 1), (5, 6), (6, 1), (6, 6)]
    assert not got.D[1].any() and got.wt[1] == 0
    # no key in common
    assert check(A[ka < 3], B, ncols, c0, b, 0, ncols).count == 0


def test_b_zero_meets_every_row():
    ncols = 70
    A, B = g.random_words(13, ncols, 5), g.random_words(17, ncols, 6)
    got = check(A, B, ncols, 33, 0, 5, 69)
    assert got.count == 13 * 17 and np.array_equal(got.ia, np.repeat(np.arange(13), 17)) and np.array_equal(got.ib, np.tile(np.arange(17), 13))


def test_a_self_join_gives_all_ordered_pairs():
    ncols, c0, b = 100, 10, 3
    A = g.random_words(60, ncols, 7)
    got = check(A, A, ncols, c0, b, 0, ncols)
    sizes = np.unique(keys(A, c0, b), return_counts=True)[1]
    assert got.count == int((sizes * sizes).sum())
    same = got.ia == got.ib
    assert same.sum() == 60 and not got.D[same].any()


def test_weights_for_ranges_inside_words():
    ncols = 200
    D = g.random_words(40, ncols, 8)
    bits = g.words_to_bits(D, ncols)
    for wc0, wc1 in ((0, 0), (200, 200), (0, 200), (5, 6), (3, 61), (63, 65), (60, 140), (64, 128), (1, 199), (129, 200), (191, 193)):
        assert np.array_equal(jr.weights(D, wc0, wc1), bits[:, wc0:wc1].sum(axis=1)), (wc0, wc1)


def test_the_count_of_random_keys_is_near_its_mean():
    """the pair indicators are pairwise independent: the variance of the count is NA NB p (1 - p) with p = 2^-b"""
    for b in (8, 12):
        N = 3 << b
        rng = np.random.default_rng(b)
        count = jr.pair_count(rng.integers(0, 1 << b, N), rng.integers(0, 1 << b, N))
        mean = N * N / (1 << b)
        assert abs(count - mean) <= 6 * np.sqrt(mean)
