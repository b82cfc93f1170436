"""The yardstick of the LF2 tests (tests/lf2_ref.py) against the definition of include/m4ri_hip_lf2.h on small pools: classes in
ascending key, inside a class the pairs of rows lo < hi ordered by (hi, lo), D = P[hi] ^ P[lo] with the excess bits zero.  No device
and nothing of the library is needed."""
import numpy as np
import pytest

import gf2util as g
import lf2_ref as lf


def key_by_bits(words, i, c0, b):
    return sum(((int(words[i, (c0 + j) >> 6]) >> ((c0 + j) & 63)) & 1) << j for j in range(b))


def by_definition(words, ncols, c0, b):
    n = words.shape[0]
    classes = {}
    for i in range(n):
        classes.setdefault(key_by_bits(words, i, c0, b), []).append(i)      # members in ascending row order
    lo, hi = [], []
    for v in sorted(classes):
        rows = classes[v]
        for x in range(len(rows)):
            for y in range(x):
                lo.append(rows[y])
                hi.append(rows[x])
    D = np.zeros((len(lo), words.shape[1]), dtype=np.uint64)
    for j, (a, c) in enumerate(zip(lo, hi)):
        D[j] = words[a] ^ words[c]
    if ncols % 64 and D.shape[1]:
        D[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    order = [i for v in sorted(classes) for i in classes[v]]
    skeys = [v for v in sorted(classes) for _ in classes[v]]
    return order, skeys, lo, hi, D


@pytest.mark.parametrize("b", [0, 2, 5, 8, 11])
@pytest.mark.parametrize("N", [0, 1, 2, 7, 50, 200, 300])
def test_the_vectorised_round_is_the_definition(N, b):
    ncols, c0 = 130, 59           # b = 8, 11: the window crosses a word boundary
    words = g.random_words(N, ncols, 1000 * b + N)
    order, skeys, lo, hi, D = by_definition(words, ncols, c0, b)
    got_order, got_keys = lf.class_sort(words, c0, b)
    assert got_order.dtype == np.int32 and list(got_order) == order and list(got_keys) == skeys
    want = lf.lf2(words, ncols, c0, b)
    assert want.count == len(lo) and list(want.lo) == lo and list(want.hi) == hi
    assert np.array_equal(want.D, D)
    assert all(a < c for a, c in zip(want.lo, want.hi))
    if len(lo):
        assert not lf.keys(want.D, c0, b).any()                    # the window of D is zero
    for limit in (0, 1, len(lo) // 2, len(lo), len(lo) + 5):       # the cut form gives a prefix
        cut = lf.lf2(words, ncols, c0, b, limit=limit)
        n = min(limit, len(lo))
        assert cut.count == len(lo) and list(cut.lo) == lo[:n] and list(cut.hi) == hi[:n] and np.array_equal(cut.D, D[:n])


def test_one_class_and_distinct_keys():
    k = np.zeros(70000, dtype=np.int64)
    assert lf.pair_count(k) == 2449965000 > 1 << 31
    lo, hi = lf.pairs(k, limit=7)
    assert list(lo) == [0, 0, 1, 0, 1, 2, 0] and list(hi) == [1, 2, 2, 3, 3, 3, 4]
    assert lf.pair_count(np.arange(1000)[::-1]) == 0 and len(lf.pairs(np.arange(1000)[::-1])[0]) == 0


@pytest.mark.parametrize("b", [8, 12, 16])
def test_a_pool_of_three_rows_per_class_keeps_its_size(b):
    """random keys: a class of n members gives n (n - 1) / 2 rows, a Poisson class size of mean m gives m^2 / 2 per class, that is
    count / N = m / 2: 1.0 at N = 2 * 2^b and 1.5 at N = 3 * 2^b.  Per class the variance of n (n - 1) / 2 is m^3 + m^2 / 2, so the
    standard deviation of the count is sqrt(10.5 N) = 3.3 sqrt(N) at m = 3 and less at m = 2: three of them are allowed."""
    rng = np.random.default_rng(b)
    for m in (2, 3):
        N = m << b
        k = rng.integers(0, 1 << b, N)
        count = lf.pair_count(k)
        assert abs(count - N * (N - 1) / 2 / (1 << b)) <= 10 * np.sqrt(N), (m, count / N)
        assert len(lf.pairs(k)[0]) == count
        assert 4 <= np.unique(k, return_counts=True)[1].max() <= 16
