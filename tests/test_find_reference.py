"""The yardstick of the row lookup (tests/find_ref.py) against second definitions, on the CPU: a brute-force double loop over bits on
pools of up to 200 rows; for A is B the rep of the yardstick of the duplicate removal (tests/unique_ref.py) and the class sizes of
numpy.unique; and every bit outside the range flipped, which must not move the result.  No library, no device."""
import numpy as np
import pytest

import find_ref as fr
import gf2util as g
import unique_ref as ur

CASES = [(1, 0, 1), (64, 0, 64), (65, 0, 65), (65, 64, 65), (130, 1, 129), (200, 57, 57), (200, 57, 87), (200, 57, 200), (200, 63, 193),
         (257, 63, 257), (300, 128, 192), (300, 0, 300)]


def pools(ncols, c0, c1, na, nb, seed):
    """B drawn from a dictionary of about nb / 3 values, A half from B's dictionary and half fresh; junk outside the range"""
    rng = np.random.default_rng(seed)
    dictionary = g.random_words(max(nb // 3, 1) + max(na // 2, 1), ncols, seed)
    known = max(nb // 3, 1)
    b = dictionary[rng.integers(0, known, nb)].copy()
    a = dictionary[np.where(rng.integers(0, 2, na) == 1, rng.integers(0, known, na), known + rng.integers(0, len(dictionary) - known, na))].copy()
    for words in (a, b):                                                                # junk in every column outside the range
        bits = g.words_to_bits(words, ncols) if len(words) else np.zeros((0, ncols), dtype=np.uint8)
        junk = rng.integers(0, 2, bits.shape, dtype=np.uint8)
        bits[:, :c0], bits[:, c1:] = junk[:, :c0], junk[:, c1:]
        if len(words):
            words[:] = g.bits_to_words(bits)
    return a, b


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_the_yardstick_against_a_double_loop(case):
    ncols, c0, c1 = case
    for na, nb in ((0, 0), (0, 5), (5, 0), (1, 1), (2, 3), (57, 200), (200, 57), (200, 200)):
        a, b = pools(ncols, c0, c1, na, nb, 11 + na + 3 * nb)
        ba = g.words_to_bits(a, ncols)[:, c0:c1] if na else np.zeros((0, c1 - c0), dtype=np.uint8)
        bb = g.words_to_bits(b, ncols)[:, c0:c1] if nb else np.zeros((0, c1 - c0), dtype=np.uint8)
        got = fr.find_rows(a, b, c0, c1)
        idx, mult = [], []
        for i in range(na):
            equal = [j for j in range(nb) if np.array_equal(ba[i], bb[j])]
            idx.append(equal[0] if equal else -1)
            mult.append(len(equal))
        assert got.idx.tolist() == idx and got.mult.tolist() == mult and got.count == sum(1 for x in idx if x >= 0)
        assert got.idx.dtype == got.mult.dtype == np.int32
        if c0 == c1 and nb:
            assert idx == [0] * na and mult == [nb] * na
        if na >= 57 and nb >= 57 and c1 - c0 >= 20:
            assert 0 < got.count < na and max(mult) > 1                                # both branches, and classes of several members


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_a_is_b_gives_rep_and_class_sizes(case):
    ncols, c0, c1 = case
    for n in (1, 2, 57, 200):
        _, b = pools(ncols, c0, c1, 0, n, 5 + n)
        got = fr.find_rows(b, b, c0, c1)
        assert np.array_equal(got.idx, ur.everything(b, c0, c1).rep) and got.count == n
        values, inverse, sizes = np.unique(ur.range_words(b, c0, c1), axis=0, return_inverse=True, return_counts=True)
        assert np.array_equal(got.mult, sizes[inverse.reshape(-1)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_bits_outside_the_range_do_not_count(case):
    ncols, c0, c1 = case
    a, b = pools(ncols, c0, c1, 150, 150, 77)
    want = fr.find_rows(a, b, c0, c1)
    outside = np.ones(ncols, dtype=np.uint8)
    outside[c0:c1] = 0
    flip = g.bits_to_words(np.tile(outside, (150, 1)))
    for fa, fb in ((a ^ flip, b), (a, b ^ flip), (a ^ flip, b ^ flip)):
        got = fr.find_rows(fa, fb, c0, c1)
        assert np.array_equal(got.idx, want.idx) and np.array_equal(got.mult, want.mult) and got.count == want.count
    # excess bits of the last word too
    top = a.copy()
    if ncols % 64:
        top[:, -1] ^= np.uint64(((1 << 64) - 1) ^ ((1 << (ncols % 64)) - 1))
    assert np.array_equal(fr.find_rows(top, b, c0, c1).idx, want.idx)
    if c1 - c0 >= 2:                                                                    # ... and one inside it does
        inside = a.copy()
        inside[:, c0 // 64] ^= np.uint64(1 << (c0 % 64))
        assert not np.array_equal(fr.find_rows(inside, b, c0, c1).idx, want.idx)
