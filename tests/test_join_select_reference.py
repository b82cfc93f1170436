"""The yardstick of the weight-filtered join (tests/join_select_ref.py) against the definition of include/m4ri_hip_join_select.h, on the
CPU: a plain double loop over all NA * NB pairs of small pools, ordered by (key, ia, ib), the weights counted bit by bit and the window
applied pair by pair.  No library, no device."""
import numpy as np
import pytest

import gf2util as g
import join_select_ref as js
from test_join_reference import set_keys


def by_definition(A, B, ncols, c0, b, wc0, wc1, wlo, whi):
    to_bits = lambda w: g.words_to_bits(w, ncols) if len(w) else np.zeros((0, ncols), dtype=np.uint8)  # noqa: E731
    bits_a, bits_b = to_bits(A), to_bits(B)
    key = lambda bits, i: sum(int(bits[i, c0 + j]) << j for j in range(b))  # noqa: E731
    pairs = sorted((key(bits_a, i), i, j) for i in range(len(A)) for j in range(len(B)) if key(bits_a, i) == key(bits_b, j))
    found = []
    for _, i, j in pairs:
        d = bits_a[i] ^ bits_b[j]
        w = sum(int(d[c]) for c in range(wc0, wc1))
        if wlo <= w <= whi:
            found.append((i, j, d, w))
    return len(pairs), found


def check(A, B, ncols, c0, b, wc0, wc1, wlo, whi):
    count, found = by_definition(A, B, ncols, c0, b, wc0, wc1, wlo, whi)
    for limit in (None, 0, 1, len(found) // 2, len(found), len(found) + 3):
        got = js.select(A, B, ncols, c0, b, wc0, wc1, wlo, whi, limit=limit)
        n = len(found) if limit is None else min(limit, len(found))
        assert got.count == count and got.hits == len(found) and len(got.ia) == len(got.ib) == len(got.wt) == len(got.D) == n
        assert [(int(i), int(j), int(w)) for i, j, w in zip(got.ia, got.ib, got.wt)] == [(i, j, w) for i, j, _, w in found[:n]]
        if n:
            assert np.array_equal(g.words_to_bits(got.D, ncols), np.array([d for _, _, d, _ in found[:n]]))
    return count, len(found)


CASES = [(130, 60, 9, 3, 127), (200, 0, 4, 64, 128), (64, 37, 5, 0, 64), (65, 64, 1, 10, 11), (256, 100, 30, 70, 200), (130, 121, 9, 0, 130),
         (100, 10, 3, 40, 40)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-b%d-w%d-%d" % c)
def test_random_pools_against_the_definition(case):
    ncols, c0, b, wc0, wc1 = case
    rng = np.random.default_rng(ncols + b)
    width = wc1 - wc0
    some = 0
    for NA, NB in ((0, 5), (5, 0), (1, 1), (37, 90), (80, 41)):
        values = rng.integers(0, 1 << b, 6)
        A = set_keys(g.random_words(NA, ncols, 1 + NA), c0, b, values[rng.integers(0, 6, NA)])
        B = set_keys(g.random_words(NB, ncols, 2 + NB), c0, b, values[rng.integers(0, 6, NB)])
        for wlo, whi in ((0, 0), (0, width // 2), (width // 2, width // 2), (width // 2 + 1, width + 9), (0, width), (1, 1 << 30)):
            count, hits = check(A, B, ncols, c0, b, wc0, wc1, wlo, whi)
            assert hits <= count and (NA and NB or count == 0)
            if (wlo, whi) == (0, width):
                assert hits == count                               # every pair
            if width == 0:
                assert hits == (count if wlo == 0 else 0)          # an empty range weighs 0
            some += 0 < hits < count
    assert some >= 1 or width <= 1                                  # a window that cuts the pairs in two was among them


def test_the_hits_keep_the_order_of_the_join():
    """two classes; the hits are picked by planted rows: A is zero on the range, so the weight of a pair is that of its row of B"""
    ncols, c0, b, wc0, wc1 = 130, 5, 6, 64, 130
    ka, kb = np.array([9, 4, 9, 4, 4]), np.array([4, 9, 9, 4, 4, 9])
    A = set_keys(np.zeros((5, 3), dtype=np.uint64), c0, b, ka)
    B = set_keys(np.zeros((6, 3), dtype=np.uint64), c0, b, kb)
    B[[0, 2, 4], 1] = np.uint64(0b111)         # weight 3 on the range: rows 0, 4 of key 4, row 2 of key 9
    got = js.select(A, B, ncols, c0, b, wc0, wc1, 3, 3)
    assert got.count == 3 * 3 + 2 * 3 and got.hits == 3 * 2 + 2 * 1
    assert list(zip(got.ia, got.ib)) == [(1, 0), (1, 4), (3, 0), (3, 4), (4, 0), (4, 4), (0, 2), (2, 2)]
    assert check(A, B, ncols, c0, b, wc0, wc1, 3, 3) == (15, 8)
    assert check(A, B, ncols, c0, b, wc0, wc1, 0, 2) == (15, 7)


def test_a_self_join():
    ncols, c0, b = 100, 10, 3
    A = g.random_words(40, ncols, 7)
    count, hits = check(A, A, ncols, c0, b, 20, 90, 0, 0)
    assert hits == 40                      # only (i, i): a zero row
