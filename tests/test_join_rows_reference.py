"""The yardstick of the grouping and of the wide join (tests/join_rows_ref.py) against a plain double loop over bits, on pools of up to
40 rows; against the yardsticks of the row sort, the duplicate removal and the row lookup for what the header says of them; and every
bit outside the range flipped, which must not move the pairs.  No library, no device."""
import numpy as np
import pytest

import find_ref as fr
import gf2util as g
import join_rows_ref as jr
import unique_ref as ur
from test_find_reference import pools

CASES = [(1, 0, 1), (64, 0, 64), (65, 64, 65), (130, 1, 129), (200, 0, 0), (200, 5, 35), (200, 37, 82), (200, 64, 128), (200, 0, 200),
         (257, 63, 257)]
WEIGHTS = lambda ncols, c0, c1: [(0, ncols), (7 % (ncols + 1), 7 % (ncols + 1)), (c0, c1), (c0 // 2, min(ncols, c1 + 3))]  # noqa: E731


def bits_of(words, ncols):
    return g.words_to_bits(words, ncols) if len(words) else np.zeros((0, ncols), dtype=np.uint8)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_the_join_against_a_double_loop(case):
    ncols, c0, c1 = case
    for na, nb in ((0, 0), (0, 5), (5, 0), (1, 1), (2, 3), (17, 40), (40, 17), (40, 40)):
        a, b = pools(ncols, c0, c1, na, nb, 21 + na + 3 * nb)
        ba, bb = bits_of(a, ncols), bits_of(b, ncols)
        pairs = [(i, j) for i in range(na) for j in range(nb) if np.array_equal(ba[i, c0:c1], bb[j, c0:c1])]
        for wc0, wc1 in WEIGHTS(ncols, c0, c1):
            for cap in (None, 0, 1, len(pairs) - 1, len(pairs), len(pairs) + 3):
                if cap is not None and cap < 0:
                    continue
                got = jr.join_rows(a, b, ncols, c0, c1, wc0, wc1, cap)
                kept = pairs if cap is None else pairs[:cap]
                assert got.count == len(pairs)
                assert got.ia.tolist() == [i for i, _ in kept] and got.ib.tolist() == [j for _, j in kept]
                assert got.ia.dtype == got.ib.dtype == got.wt.dtype == np.int32 and got.d.dtype == np.uint64
                x = np.array([ba[i] ^ bb[j] for i, j in kept], dtype=np.uint8).reshape(len(kept), ncols)
                assert np.array_equal(bits_of(got.d, ncols), x) and got.d.shape == (len(kept), (ncols + 63) // 64)
                assert got.wt.tolist() == [int(r[wc0:wc1].sum()) for r in x]
                if ncols % 64 and len(kept):
                    assert not (got.d[:, -1] >> np.uint64(ncols % 64)).any()               # the excess bits are zero
        if c0 == c1:
            assert len(pairs) == na * nb
        if na == nb == 40 and c1 - c0 >= 20:
            assert 0 < len(pairs) and len({i for i, _ in pairs}) < na                      # matches and rows without a partner


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_the_grouping_against_a_double_loop(case):
    ncols, c0, c1 = case
    for n in (0, 1, 2, 17, 40):
        _, p = pools(ncols, c0, c1, 0, n, 31 + n)
        bp = bits_of(p, ncols)[:, c0:c1]
        rep = [min(j for j in range(n) if np.array_equal(bp[i], bp[j])) for i in range(n)]
        order = sorted(range(n), key=lambda i: (rep[i], i))
        head = [order.index(rep[i]) for i in order]
        got = jr.group_rows(p, c0, c1)
        assert got[0].tolist() == order and got[1].tolist() == head and got[0].dtype == got[1].dtype == np.int32
        # what the header says of the other entries: the classes of the row sort, the rep of the duplicate removal, the sizes of the lookup
        every = ur.everything(p, c0, c1)
        assert got[0][got[1]].tolist() == every.rep[got[0]].tolist()
        sizes = np.bincount(got[1], minlength=n)[got[1]] if n else np.zeros(0, dtype=np.int64)
        assert sizes.tolist() == fr.find_rows(p, p, c0, c1).mult[got[0]].tolist()
        by_value = {tuple(sorted(every.order[every.head == h].tolist())) for h in set(every.head.tolist())}
        by_rep = {tuple(got[0][got[1] == h].tolist()) for h in set(got[1].tolist())}
        assert by_value == by_rep                                                          # exactly the classes of the row sort
        if c0 == c1 and n:
            assert order == list(range(n)) and head == [0] * n
        # (c) of the header: with A == B, the partners of the lowest row of a class are the class in the grouping's order
        j = jr.join_rows(p, p, ncols, c0, c1)
        for r in set(rep):
            assert j.ib[j.ia == r].tolist() == [i for i in order if rep[i] == r]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_bits_outside_the_range_do_not_count(case):
    ncols, c0, c1 = case
    a, b = pools(ncols, c0, c1, 40, 40, 77)
    want = jr.join_rows(a, b, ncols, c0, c1)
    outside = np.ones(ncols, dtype=np.uint8)
    outside[c0:c1] = 0
    flip = g.bits_to_words(np.tile(outside, (40, 1)))
    for fa, fb in ((a ^ flip, b), (a, b ^ flip), (a ^ flip, b ^ flip)):
        got = jr.join_rows(fa, fb, ncols, c0, c1)
        assert got.count == want.count and np.array_equal(got.ia, want.ia) and np.array_equal(got.ib, want.ib)
    assert np.array_equal(jr.group_rows(b ^ flip, c0, c1)[0], jr.group_rows(b, c0, c1)[0])
    top = a.copy()                                                                         # dirty excess bits: same pairs, clean rows
    if ncols % 64:
        top[:, -1] ^= np.uint64(((1 << 64) - 1) ^ ((1 << (ncols % 64)) - 1))
    got = jr.join_rows(top, b, ncols, c0, c1)
    assert np.array_equal(got.ia, want.ia) and np.array_equal(got.d, want.d)
