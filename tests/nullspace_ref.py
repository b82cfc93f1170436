"""Inputs and expectations of the null space tests (tests/test_nullspace_host.py, tests/test_gpu_nullspace.py); numpy only.

The contract: A is m x n of rank r with pivot columns p_0 < ... < p_{r-1} and free columns f_0 < ... <
f_{n-r-1}, E its reduced row echelon form; K is n x (n - r), row f_j = the unit vector e_j, row p_i = (E[i][f_j])_j.

with_pivots builds a matrix WITH a given pivot set and reads K straight off the E it was built from, so the expectation rests on
neither the library nor the oracle; from_rref gives the same basis from a reduced echelon form somebody computed."""
import functools

import numpy as np

import gf2util as g


def basis_bits(e_bits, pivots, n):
    """K as (n, n - r) uint8 from the rows of the reduced echelon form (r x n uint8) and its pivot columns"""
    pivots = np.asarray(pivots, dtype=np.int64)
    r = len(pivots)
    free = np.setdiff1d(np.arange(n), pivots)
    k = np.zeros((n, n - r), dtype=np.uint8)
    k[free, np.arange(n - r)] = 1
    if r:
        k[pivots, :] = e_bits[:r][:, free]
    return k


def to_words(k_bits):
    """(n, d) uint8 -> (n, width(d)) words; d == 0 gives an (n, 0) array"""
    if k_bits.shape[1] == 0:
        return np.zeros((k_bits.shape[0], 0), dtype=np.uint64)
    return g.bits_to_words(k_bits)


@functools.lru_cache(maxsize=None)
def _with_pivots(m, n, S, seed):
    rng = np.random.default_rng(seed)
    piv = np.asarray(S, dtype=np.int64)
    r = len(piv)
    assert r <= m and r <= n and np.all(np.diff(piv) > 0) and (r == 0 or (piv[0] >= 0 and piv[-1] < n))
    free = np.setdiff1d(np.arange(n), piv)
    e = np.zeros((r, n), dtype=np.uint8)
    e[np.arange(r), piv] = 1
    if r and len(free):  # random bits at the free columns right of each pivot
        e[:, free] = rng.integers(0, 2, size=(r, len(free)), dtype=np.uint8) & (free[None, :] > piv[:, None])
    # M: full column rank -- a random unit lower triangular block on random rows, the rows shuffled
    mm = rng.integers(0, 2, size=(m, r), dtype=np.uint8)
    mm[:r] = np.tril(mm[:r], -1) + np.eye(r, dtype=np.uint8)
    mm = mm[rng.permutation(m)]
    a = np.zeros((m, n), dtype=np.uint8)
    a[:, piv] = mm  # E's pivot columns are unit vectors
    if r and len(free):
        a[:, free] = np.rint(mm.astype(np.float32) @ e[:, free].astype(np.float32)).astype(np.int64) & 1  # sums < 2^24: exact
    a_words, k_words = g.bits_to_words(a), to_words(basis_bits(e, piv, n))
    a_words.setflags(write=False)
    k_words.setflags(write=False)
    return a_words, k_words


def with_pivots(m, n, S, seed):
    """-> (A words, K words): A = M E is m x n with pivot columns S (M of full column rank), K the expected basis read off E.
    The arrays are shared between tests and read-only: copy before handing them to something that writes."""
    return _with_pivots(m, n, tuple(int(c) for c in S), seed)


def from_rref(e_words, pivots, n):
    """the same basis from a reduced echelon form (words; rows 0 .. r - 1 are the pivot rows) and its pivot columns"""
    r = len(pivots)
    return to_words(basis_bits(g.words_to_bits(np.ascontiguousarray(e_words[:max(r, 1)]), n), pivots, n))


def no_excess(k_words, d):
    return d % 64 == 0 or k_words.shape[1] == 0 or not np.any(k_words[:, -1] >> np.uint64(d % 64))


ONE_PER_WORD = [63, 64, 130, 200, 260, 330, 400, 450, 520, 580, 650, 710, 770, 840, 900]  # + one in [960, 1000)


def patterns():
    """(name, m, n, pivot columns): the smallest shapes at which the column compress can go wrong"""
    out = []
    for n, m in ((130, 140), (300, 320)):  # n = 130: the single-workgroup elimination; 300: the blocked one
        for d in (1, 63, 64, 65, 129):
            out.append(("pivots_first_n%d_d%d" % (n, d), m, n, range(n - d)))
    for r in (170, 236):
        out.append(("pivots_last_r%d" % r, 320, 300, range(300 - r, 300)))
    for n in (129, 640):
        out.append(("alternating_n%d" % n, n // 2 + 10, n, range(1, n, 2)))
    for bit in (0, 63, 29):  # output word 0 draws from 64 source words, word 1 from 2
        n = 64 * 66
        out.append(("one_free_per_word_bit%d" % bit, 4200, n, np.setdiff1d(np.arange(n), np.arange(bit, n, 64))))
    out.append(("one_pivot_per_word", 20, 1000, ONE_PER_WORD + [999]))
    out.append(("one_pivot_per_word_last_free", 20, 1000, ONE_PER_WORD + [970]))  # column 999 free, in a ragged last word
    out.append(("n1_zero", 1, 1, []))
    out.append(("n1_one", 1, 1, [0]))
    out.append(("n37", 8, 37, [1, 5, 6, 20, 36]))
    out.append(("rank0", 5, 130, []))
    return out
