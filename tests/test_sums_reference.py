"""The yardstick of the subset-sum tests (tests/sums_ref.py) against the definition of include/m4ri_hip_sums.h, on the CPU: the order is
itertools.combinations sorted by the reversed tuple, the rank is the combinatorial number system, the sums and weights are counted
bit by bit.  The host routines of the built library (gf2_subset_count, gf2_subset_rank, gf2_subset_unrank) round-trip against it
through ctypes.  No device."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import gf2util as g
import sums_ref as sr

SMALL = [(n, p) for p in range(1, 5) for n in range(p, 13)]


@pytest.mark.parametrize("n,p", SMALL)
def test_the_order_is_combinations_sorted_by_the_reversed_tuple(n, p):
    want = sorted(itertools.combinations(range(n), p), key=lambda c: tuple(reversed(c)))
    got = sr.subsets(n, p)
    assert got.shape == (math.comb(n, p), p) == (sr.count(n, p), p) and [tuple(r) for r in got] == want
    # the rank formula, and unrank and successor, which make the windows of the lists that are too long to enumerate
    c = sr.unrank(0, p)
    for r, row in enumerate(want):
        assert sr.rank(row) == r == sum(math.comb(ci, i + 1) for i, ci in enumerate(row))
        assert sr.unrank(r, p) == row == c
        c = sr.successor(c)
    if p == 2:
        assert all(sr.rank((a, b)) == b * (b - 1) // 2 + a for a, b in want)
    # a list over n rows is the beginning of the list over n + 1
    assert np.array_equal(sr.subsets(n + 1, p)[:len(want)], got)
    for rank0, cnt in ((0, 0), (0, 1), (len(want) - 1, 1), (len(want) // 3, len(want) // 2), (len(want), 0)):
        assert [tuple(r) for r in sr.subsets(n, p, rank0, cnt)] == want[rank0:rank0 + cnt]


def test_n_below_p_has_no_subset():
    for p in range(1, 5):
        for n in range(p):
            assert sr.count(n, p) == 0 and sr.subsets(n, p).shape == (0, p)


def test_windows_of_long_lists_walk_from_an_unranked_start(monkeypatch):
    """the route for lists that are not enumerated gives what the enumeration gives"""
    for n, p in ((40, 2), (20, 3), (14, 4), (50, 1)):
        whole = sr.subsets(n, p).copy()
        monkeypatch.setattr(sr, "ENUMERATE_UP_TO", 0)
        for rank0, cnt in ((0, len(whole)), (7, 30), (len(whole) - 5, 5), (3, 0)):
            assert np.array_equal(sr.subsets(n, p, rank0, cnt), whole[rank0:rank0 + cnt])
        monkeypatch.undo()
    big = sr.subsets(131072, 2, (1 << 32) - 3, 6)
    assert [sr.rank(tuple(int(x) for x in r)) for r in big] == list(range((1 << 32) - 3, (1 << 32) + 3))
    assert sr.unrank(1 << 62, 4) == sr.successor(sr.unrank((1 << 62) - 1, 4))


@pytest.mark.parametrize("ncols", [1, 64, 70, 130])
def test_sums_and_weights_bit_by_bit(ncols):
    n = 9
    S = g.random_words(n, ncols, ncols)
    base = g.random_words(1, ncols, ncols + 1)
    sbits, bbits = g.words_to_bits(S, ncols), g.words_to_bits(base, ncols)[0]
    for p in range(1, 5):
        for b in (None, base):
            wc0, wc1 = ncols // 3, ncols - ncols // 4
            got = sr.sums(S, ncols, p, base=b, wc0=wc0, wc1=wc1)
            want = sorted(itertools.combinations(range(n), p), key=lambda c: c[::-1])
            assert [tuple(r) for r in got.idx] == want and got.idx.dtype == np.int32 and got.wt.dtype == np.int32
            bits = np.array([np.bitwise_xor.reduce(sbits[list(c)], axis=0) ^ (bbits if b is not None else 0) for c in want], dtype=np.uint8)
            assert np.array_equal(g.words_to_bits(got.D, ncols), bits)
            assert np.array_equal(got.wt, bits[:, wc0:wc1].sum(axis=1))
            part = sr.sums(S, ncols, p, base=b, rank0=2, cnt=len(want) - 3, wc0=wc0, wc1=wc1)
            assert np.array_equal(part.D, got.D[2:-1]) and np.array_equal(part.idx, got.idx[2:-1]) and np.array_equal(part.wt, got.wt[2:-1])


# ---- the host routines of the library ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L(built):
    import m4ri_rust_amd as pkg
    return pkg._lib.lib()


def lib_rank(L, c):
    return L.gf2_subset_rank((ctypes.c_int * len(c))(*c), len(c))


def lib_unrank(L, r, p):
    c = (ctypes.c_int * 4)(-7, -7, -7, -7)
    rc = L.gf2_subset_unrank(r, p, c)
    return rc, tuple(c)


def test_library_count(L):
    for p in range(1, 5):
        for n in range(0, 40):
            assert L.gf2_subset_count(n, p) == sr.count(n, p)
        assert L.gf2_subset_count(-3, p) == 0
    assert L.gf2_subset_count(131072, 2) == 131072 * 131071 // 2 == math.comb(131072, 2)
    assert L.gf2_subset_count((1 << 31) - 1, 1) == (1 << 31) - 1
    assert L.gf2_subset_count((1 << 31) - 1, 2) == math.comb((1 << 31) - 1, 2) < 1 << 62
    for p in (3, 4):
        last = p
        while math.comb(2 * last, p) <= 1 << 62:
            last *= 2
        lo, hi = last, 2 * last         # the largest n whose C(n, p) stays below 2^62, by bisection on exact integers
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if math.comb(mid, p) <= 1 << 62 else (lo, mid)
        assert math.comb(lo, p) < 1 << 62 < math.comb(lo + 1, p)
        assert L.gf2_subset_count(lo, p) == math.comb(lo, p) and L.gf2_subset_count(lo + 1, p) == -1
        assert L.gf2_subset_count((1 << 31) - 1, p) == -1
    for p in (0, -1, 5, 1 << 20):
        assert L.gf2_subset_count(10, p) == -1


def test_library_rank_and_unrank_round_trip(L):
    for n, p in SMALL:
        for r, row in enumerate(sr.subsets(n, p)):
            c = tuple(int(x) for x in row)
            assert lib_rank(L, c) == r and lib_unrank(L, r, p) == (0, c + (-7,) * (4 - p))
    rng = np.random.default_rng(5)
    tops = {1: (1 << 31) - 1, 2: (1 << 31) - 1, 3: 3024617, 4: 102570}       # the largest n the library takes for every p
    for p, n in tops.items():
        assert L.gf2_subset_count(n, p) >= 0
        total = math.comb(n, p)
        ranks = [0, 1, total - 1, total // 2, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
        ranks += [int(x) for x in rng.integers(0, min(total, (1 << 62) - 1), 200)]
        for r in ranks:
            if r >= total:
                continue
            c = sr.unrank(r, p)
            assert c[-1] < n and lib_unrank(L, r, p) == (0, c + (-7,) * (4 - p)) and lib_rank(L, c) == r, (p, r)
    assert L.gf2_subset_count(131072, 2) == lib_rank(L, (131070, 131071)) + 1
    assert lib_unrank(L, math.comb(131072, 2) - 1, 2)[1][:2] == (131070, 131071)


def test_library_refuses_bad_subsets_and_ranks(L):
    for c in ((-1,), (3, 3), (4, 3), (0, 1, 1), (0, 2, 1, 5), (5, 4, 3, 2), (-1, 0)):
        assert lib_rank(L, c) == -1, c
    assert L.gf2_subset_rank(None, 2) == -1
    assert L.gf2_subset_rank((ctypes.c_int * 5)(0, 1, 2, 3, 4), 5) == -1 and L.gf2_subset_rank((ctypes.c_int * 1)(0), 0) == -1
    assert lib_rank(L, (0, 1, 2, 102570)) == -1 and lib_rank(L, (0, 1, 2, 102569)) == math.comb(102569, 4)   # C(c_p + 1, p) past 2^62
    assert lib_rank(L, (0, 1, (1 << 31) - 1)) == -1
    for r, p in ((-1, 2), (1 << 62, 4), ((1 << 63) - 1, 3), (0, 0), (0, 5), (1 << 31, 1), (1 << 61, 2)):       # the last two: c_p past an int
        assert lib_unrank(L, r, p) == (-1, (-7,) * 4), (r, p)
    assert L.gf2_subset_unrank(0, 2, None) == -1
    assert lib_unrank(L, (1 << 31) - 1, 1) == (0, ((1 << 31) - 1, -7, -7, -7))
