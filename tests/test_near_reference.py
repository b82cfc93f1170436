"""The yardstick of the Hamming-distance search (tests/near_ref.py) against the definition of include/m4ri_hip_near.h, on the CPU: a plain
double loop over all NA * NB pairs of small pools, the distances counted bit by bit, the flags and the window applied pair by pair; and
against the yardstick of the weight-filtered join (tests/join_select_ref.py), whose pairs with b == 0 are those of flags == 0.  No
library, no device."""
import numpy as np
import pytest

import gf2util as g
import join_select_ref as js
import near_ref as nr


def bits_of(words, ncols):
    return g.words_to_bits(words, ncols) if len(words) and ncols else np.zeros((len(words), ncols), dtype=np.uint8)


def admits(i, j, flags):
    if flags & nr.UPPER:
        return i < j
    if flags & nr.OFF_DIAGONAL:
        return i != j
    return True


def by_definition(A, B, ncols, wc0, wc1, wlo, whi, flags):
    ba, bb = bits_of(A, ncols), bits_of(B, ncols)
    found = []
    for i in range(len(A)):
        for j in range(len(B)):
            d = ba[i] ^ bb[j]
            w = sum(int(d[c]) for c in range(wc0, wc1))
            if admits(i, j, flags) and wlo <= w <= whi:
                found.append((i, j, d, w))
    return found


def nearest_by_definition(A, B, ncols, wc0, wc1, flags):
    ba, bb = bits_of(A, ncols), bits_of(B, ncols)
    idx, dist = [], []
    for i in range(len(A)):
        best = (-1, -1)
        for j in range(len(B)):
            w = sum(int(ba[i, c] ^ bb[j, c]) for c in range(wc0, wc1))
            if admits(i, j, flags) and (best[0] < 0 or w < best[1]):      # strictly less: the lowest row among equals stays
                best = (j, w)
        idx.append(best[0])
        dist.append(best[1])
    return idx, dist


CASES = [(130, 3, 127), (200, 64, 128), (64, 0, 64), (65, 10, 11), (65, 60, 65), (100, 40, 40), (37, 0, 37), (1, 0, 1)]
SIZES = ((0, 5), (5, 0), (1, 1), (23, 40), (40, 23), (30, 30))
ALL_FLAGS = (0, nr.OFF_DIAGONAL, nr.UPPER, nr.OFF_DIAGONAL | nr.UPPER)


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-w%d-%d" % c)
def test_the_yardstick_against_a_double_loop(case, flags):
    ncols, wc0, wc1 = case
    width = wc1 - wc0
    for NA, NB in SIZES:
        A, B = g.random_words(NA, ncols, 1 + NA), g.random_words(NB, ncols, 2 + NB)
        if NA > 3 and NB > 8:
            B[7] = A[2]                                                   # a pair at distance 0, and ties for the nearest
            B[3] = B[7]
        d = nr.distances(A, B, ncols, wc0, wc1)
        assert d.shape == (NA, NB) and d.dtype == np.int64
        for wlo, whi in ((0, 0), (0, width // 2), (width // 2, width // 2), (width // 2 + 1, width + 9), (0, width), (1, 1 << 30)):
            found = by_definition(A, B, ncols, wc0, wc1, wlo, whi, flags)
            for limit in (None, 0, 1, len(found) // 2, len(found) + 3):
                got = nr.near_pairs(A, B, ncols, wc0, wc1, wlo, whi, flags, limit=limit)
                n = len(found) if limit is None else min(limit, len(found))
                assert got.hits == len(found) and len(got.ia) == len(got.ib) == len(got.wt) == len(got.D) == n
                assert [(int(i), int(j), int(w)) for i, j, w in zip(got.ia, got.ib, got.wt)] == [(i, j, w) for i, j, _, w in found[:n]]
                if n:
                    assert np.array_equal(bits_of(got.D, ncols), np.array([x for _, _, x, _ in found[:n]]))
            if width == 0:
                assert len(found) == (int(nr.admitted(NA, NB, flags).sum()) if wlo == 0 else 0)      # an empty range weighs 0
        idx, dist = nr.nearest(A, B, ncols, wc0, wc1, flags)
        want = nearest_by_definition(A, B, ncols, wc0, wc1, flags)
        assert (idx.tolist(), dist.tolist()) == want and idx.dtype == dist.dtype == np.int32
        if NA > 3 and NB > 8 and flags == 0 and width > 8:
            assert (idx[2], dist[2]) == (3, 0)                               # rows 3 and 7 of B tie: the lower one


@pytest.mark.parametrize("case", [(130, 3, 127), (200, 64, 128), (64, 0, 64), (65, 64, 65), (100, 40, 40), (256, 70, 200)],
                         ids=lambda c: "%d-w%d-%d" % c)
def test_no_flags_is_the_join_with_an_empty_window(case):
    """near_pairs(flags=0) against join_select_ref.select(..., c0=0, b=0, ...): every row has key 0, the pairs ordered by (ia, ib)"""
    ncols, wc0, wc1 = case
    width = wc1 - wc0
    for NA, NB in ((0, 5), (5, 0), (1, 1), (37, 90), (80, 41)):
        A, B = g.random_words(NA, ncols, 11 + NA), g.random_words(NB, ncols, 12 + NB)
        for wlo, whi in ((0, 0), (0, width // 2), (width // 2 - 3, width // 2), (width // 2 + 1, width + 9), (0, width)):
            if wlo < 0:
                continue
            for limit in (None, 7):
                want = js.select(A, B, ncols, 0, 0, wc0, wc1, wlo, whi, limit=limit)
                got = nr.near_pairs(A, B, ncols, wc0, wc1, wlo, whi, 0, limit=limit)
                assert want.count == NA * NB and got.hits == want.hits
                assert np.array_equal(got.ia, want.ia) and np.array_equal(got.ib, want.ib) and np.array_equal(got.wt, want.wt)
                assert np.array_equal(got.D, want.D)


def test_nearest_is_the_argmin_of_the_distance_table():
    ncols, wc0, wc1 = 200, 30, 170
    A, B = g.random_words(50, ncols, 5), g.random_words(70, ncols, 6)
    B[40] = B[11]                                # duplicate rows of B: ties
    B[60] = B[11]
    A[9] = B[11]
    d = nr.distances(A, B, ncols, wc0, wc1)
    idx, dist = nr.nearest(A, B, ncols, wc0, wc1)
    assert np.array_equal(idx, d.argmin(axis=1)) and np.array_equal(dist, d.min(axis=1))       # numpy's argmin: the first of equals
    assert (idx[9], dist[9]) == (11, 0)
    same = np.zeros((6, 4), dtype=np.uint64)
    idx, dist = nr.nearest(same, same, ncols, wc0, wc1)                                         # all rows equal
    assert idx.tolist() == [0] * 6 and dist.tolist() == [0] * 6
    idx, dist = nr.nearest(same, same, ncols, wc0, wc1, nr.OFF_DIAGONAL)
    assert idx.tolist() == [1, 0, 0, 0, 0, 0] and dist.tolist() == [0] * 6
    idx, dist = nr.nearest(same, same, ncols, wc0, wc1, nr.UPPER)
    assert idx.tolist() == [1, 2, 3, 4, 5, -1] and dist.tolist() == [0] * 5 + [-1]


def test_the_flags_on_a_pool_against_itself():
    ncols = 100
    A = g.random_words(40, ncols, 7)
    A[30] = A[4]                                 # a near duplicate pair
    every = nr.near_pairs(A, A, ncols, 0, ncols, 0, 0)
    assert every.hits == 42 and sorted(zip(every.ia, every.ib)) == sorted([(i, i) for i in range(40)] + [(4, 30), (30, 4)])
    off = nr.near_pairs(A, A, ncols, 0, ncols, 0, 0, nr.OFF_DIAGONAL)
    assert list(zip(off.ia, off.ib)) == [(4, 30), (30, 4)] and not off.D.any()
    for flags in (nr.UPPER, nr.UPPER | nr.OFF_DIAGONAL):
        up = nr.near_pairs(A, A, ncols, 0, ncols, 0, 0, flags)
        assert list(zip(up.ia, up.ib)) == [(4, 30)]
    # every unordered pair once: the ordered pairs are twice those and the diagonal
    n_all = nr.near_pairs(A, A, ncols, 0, ncols, 0, ncols).hits
    n_off = nr.near_pairs(A, A, ncols, 0, ncols, 0, ncols, nr.OFF_DIAGONAL).hits
    n_up = nr.near_pairs(A, A, ncols, 0, ncols, 0, ncols, nr.UPPER).hits
    assert (n_all, n_off, n_up) == (1600, 1560, 780)
    # the flags compare row numbers alone: another pool, another height
    B = g.random_words(25, ncols, 8)
    assert nr.near_pairs(A, B, ncols, 0, ncols, 0, ncols, nr.UPPER).hits == sum(max(25 - i - 1, 0) for i in range(40))
    assert nr.near_pairs(A, B, ncols, 0, ncols, 0, ncols, nr.OFF_DIAGONAL).hits == 40 * 25 - 25
    idx, dist = nr.nearest(A[:3], B[:1], ncols, 0, ncols, nr.OFF_DIAGONAL)             # a B of one row: row 0 of A has no partner
    assert idx.tolist() == [-1, 0, 0] and dist[0] == -1 and (dist[1:] >= 0).all()
