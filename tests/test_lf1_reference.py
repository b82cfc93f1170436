"""tests/lf1_ref.py against the definition of an LF1 round, without the library: a quadratic loop over rows of bits.  The partner of
row i is the LEAST j whose key equals key(i); row i survives when that j is not i (or, with keep_zero, when its key is 0, and then it
stays as it is); the survivors keep their order."""
import numpy as np
import pytest

import gf2util as g
import lf1_ref as lf


def by_definition(bits, c0, b, keep_zero):
    n = bits.shape[0]
    key = [tuple(bits[i, c0:c0 + b]) for i in range(n)]
    first = np.full(1 << b, -1, dtype=np.int64)
    src, partner, rows = [], [], []
    for i in range(n):
        j = next(j for j in range(n) if key[j] == key[i])    # the least j with the same key
        v = sum(int(x) << t for t, x in enumerate(key[i]))
        if j == i:
            first[v] = i
        if keep_zero and v == 0:
            src.append(i), partner.append(-1), rows.append(bits[i])
        elif j != i:
            src.append(i), partner.append(j), rows.append(bits[i] ^ bits[j])
    D = np.array(rows, dtype=np.uint8).reshape(len(rows), bits.shape[1])
    return first, np.array(src, dtype=np.int64), np.array(partner, dtype=np.int64), D


# (nrows, ncols, c0, b): one word; across a word boundary; up to the last column; from bit 0 of the second word; no window bit
CASES = [(40, 64, 0, 3), (200, 130, 37, 5), (150, 130, 60, 7), (150, 130, 62, 2), (300, 200, 50, 20), (90, 128, 120, 8), (90, 70, 64, 6),
         (120, 130, 64, 4), (33, 100, 17, 0), (33, 100, 100, 0), (1, 64, 3, 2), (0, 64, 3, 2), (500, 65, 63, 2), (64, 1, 0, 1)]


@pytest.mark.parametrize("keep_zero", [False, True], ids=["drop", "keep0"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-c%d-b%d" % c)
def test_reference_is_the_definition(case, keep_zero):
    nrows, ncols, c0, b = case
    rng = np.random.default_rng(nrows + 7 * c0 + b)
    bits = rng.integers(0, 2, (nrows, ncols), dtype=np.uint8)
    if b > 8 and nrows:   # few classes, so that rows meet: the window of every row is one of 6 patterns
        bits[:, c0:c0 + b] = bits[rng.integers(0, 6, nrows), c0:c0 + b]
    if nrows > 8:
        bits[nrows // 2, c0:c0 + b] = 0      # a row of key 0 ...
        bits[nrows - 1, c0:c0 + b] = 0       # ... and a later one
        bits[5] = bits[2]                    # a repeated row: a zero row in D
    words = g.bits_to_words(bits) if nrows else np.zeros((0, g.width(ncols)), dtype=np.uint64)
    first, src, partner, D = by_definition(bits, c0, b, keep_zero)
    got = lf.lf1(words, ncols, c0, b, keep_zero)
    assert got.first.dtype == np.int32 and got.src.dtype == np.int32 and got.D.dtype == np.uint64
    assert np.array_equal(got.first, first)
    assert np.array_equal(lf.class_first(words, c0, b), first)
    assert np.array_equal(got.src, src) and np.array_equal(got.partner, partner)
    assert got.D.shape == (len(src), g.width(ncols))
    if len(src):
        assert np.array_equal(g.words_to_bits(got.D, ncols), D)
    if ncols % 64 and len(src):
        assert not (got.D[:, -1] >> np.uint64(ncols % 64)).any()
    # what the definition implies
    k = lf.keys(words, c0, b)
    assert np.array_equal(k, [sum(int(x) << t for t, x in enumerate(bits[i, c0:c0 + b])) for i in range(nrows)])
    dk = lf.keys(got.D, c0, b)
    assert not dk.any()                                           # the window of every survivor is zero
    classes = len(set(k.tolist()))
    zeros = int((k == 0).sum())
    assert len(src) == nrows - classes + (1 if keep_zero and zeros else 0)
    if nrows > 8 and not keep_zero:
        at = list(src).index(5)
        assert partner[at] != 2 or not got.D[at].any()


def test_all_rows_in_one_class_and_all_keys_distinct():
    words = g.random_words(50, 128, 3)
    words[:, 0] = np.uint64(0x1234)
    r = lf.lf1(words, 128, 0, 16)
    assert np.array_equal(r.src, np.arange(1, 50)) and not r.partner.any() and r.first[0x1234] == 0 and (r.first >= 0).sum() == 1
    words[:, 0] = np.arange(50, dtype=np.uint64)[::-1]
    r = lf.lf1(words, 128, 0, 16)
    assert len(r.src) == 0 and r.D.shape == (0, 2) and np.array_equal(r.first[:50], np.arange(50)[::-1])
    r = lf.lf1(words, 128, 0, 16, keep_zero=True)
    assert list(r.src) == [49] and list(r.partner) == [-1] and np.array_equal(r.D[0], words[49])
