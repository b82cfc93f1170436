"""Independent checks of a triangular solve over GF(2), shared by tests/test_trsm_host.py, tests/test_gpu_trsm.py and
tests/golden/make_golden_trsm.py.  Nothing here calls the library under test:

  1. solve():        bit-level substitution in numpy (T as a bit matrix, one column at a time; the rows of B as words);
  2. check_product(): clean(T) * X == B0 (left) or X * clean(T) == B0 (right) through the oracle's product;
  3. closed forms:   T = identity gives X = B; T = the full triangle of ones has the bidiagonal inverse.

T is always taken as UNIT triangular: only its strict lower (upper) triangle counts."""
import numpy as np

import gf2util as g

VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (upper, right)


def name(upper, right):
    return ("upper" if upper else "lower") + "_" + ("right" if right else "left")


def b_shape(n, k, right):
    return (k, n) if right else (n, k)


def random_bits(rows, cols, seed):
    return g.words_to_bits(g.random_words(rows, cols, seed), cols)


def strict(n, upper):
    i, j = np.indices((n, n))
    return j > i if upper else j < i


def clean(tb, upper):
    """the triangle that counts, with the unit diagonal; everything else zero"""
    n = tb.shape[0]
    out = np.where(strict(n, upper), tb, 0).astype(np.uint8)
    out[np.arange(n), np.arange(n)] = 1
    return out


def dirty(tb, upper, seed, zero_diagonal=False):
    """the same strict triangle; random bits in the other triangle and on the diagonal (or a zero diagonal)"""
    n = tb.shape[0]
    out = np.where(strict(n, upper), tb, random_bits(n, n, seed)).astype(np.uint8)
    if zero_diagonal:
        out[np.arange(n), np.arange(n)] = 0
    return out


def ones(n, upper):
    return clean(np.ones((n, n), dtype=np.uint8), upper)


def _solve_left(tb, xw, upper):
    """T X = B by substitution: once row i of X is final it is added to every later row whose T has a bit in column i."""
    x = xw.copy()
    n = tb.shape[0]
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        col = tb[:, i].astype(bool)
        if upper:
            col[i:] = False
        else:
            col[:i + 1] = False
        x[col] ^= x[i]
    return x


def solve(tb, bw, rows, cols, upper, right):
    """X (words) with T X = B (right False; B is n x cols) or X T = B (right True; B is rows x n)."""
    if not right:
        return _solve_left(tb, bw, upper)
    # X T = B  <=>  T^T X^T = B^T, and T^T is triangular the other way round
    bt = g.bits_to_words(np.ascontiguousarray(g.words_to_bits(bw, cols).T))
    xt = _solve_left(np.ascontiguousarray(tb.T), bt, not upper)
    return g.bits_to_words(np.ascontiguousarray(g.words_to_bits(xt, rows).T))


def check_product(tb, xw, b0, rows, cols, upper, right):
    tw = g.bits_to_words(clean(tb, upper))
    n = tb.shape[0]
    prod = g.o_mul_fast(xw, tw, rows, n, n) if right else g.o_mul_fast(tw, xw, n, n, cols)
    assert np.array_equal(prod, b0), name(upper, right) + ": clean(T) and X do not multiply back to B"


def ones_closed_form(b0, cols, upper, right):
    """X for T = the full triangle of ones: each row (column) of B plus its neighbour"""
    b = g.words_to_bits(b0, cols)
    x = b.copy()
    if not right:
        if upper:
            x[:-1] ^= b[1:]   # X_i = B_i ^ B_{i+1}
        else:
            x[1:] ^= b[:-1]   # X_i = B_i ^ B_{i-1}
    else:
        if upper:
            x[:, 1:] ^= b[:, :-1]  # X[:, j] = B[:, j] ^ B[:, j-1]
        else:
            x[:, :-1] ^= b[:, 1:]  # X[:, j] = B[:, j] ^ B[:, j+1]
    return g.bits_to_words(x)


def no_excess(xw, cols):
    return not (cols % 64) or not (xw[:, -1] >> np.uint64(cols % 64)).any()


def check_variant(run, n, k, upper, right, seed, substitution=True):
    """run(t_words, b_words, n, rows, cols, upper, right) -> X words.  Checks 1 (if substitution), 2 and 3; returns (T bits, B0, X)."""
    rows, cols = b_shape(n, k, right)
    what = "%s n=%d k=%d" % (name(upper, right), n, k)
    tb = clean(random_bits(n, n, seed), upper)
    b0 = g.random_words(rows, cols, seed + 1)
    x = run(g.bits_to_words(tb), b0.copy(), n, rows, cols, upper, right)
    assert x.shape == b0.shape and no_excess(x, cols), what + ": excess bits set"
    if substitution:
        assert np.array_equal(x, solve(tb, b0, rows, cols, upper, right)), what + ": differs from the substitution"
    check_product(tb, x, b0, rows, cols, upper, right)
    eye = np.eye(n, dtype=np.uint8)
    assert np.array_equal(run(g.bits_to_words(eye), b0.copy(), n, rows, cols, upper, right), b0), what + ": identity"
    got = run(g.bits_to_words(ones(n, upper)), b0.copy(), n, rows, cols, upper, right)
    assert np.array_equal(got, ones_closed_form(b0, cols, upper, right)), what + ": triangle of ones"
    return tb, b0, x
