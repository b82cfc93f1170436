"""Inputs shared by the PLE / PLUQ tests (tests/test_gpu_ple.py, tests/test_gpu_ple_exact.py, tests/test_ple_oracle.py): low-rank
products and the seven structured patterns, as (m, width(n)) uint64 word arrays with zero excess bits."""
import numpy as np

import gf2util as g


def low_rank(m, n, r, seed):
    """m x n of rank r (with overwhelming probability): an m x r times an r x n random product"""
    if r == 0:
        return np.zeros((m, g.width(n)), dtype=np.uint64)
    return g.o_mul_fast(g.random_words(m, r, seed), g.random_words(r, n, seed + 1), m, r, n)


def structured(m, n):
    """zero, identity, reversed identity, repeated rows, leading zero columns, all rows equal, one sparse column"""
    yield np.zeros((m, g.width(n)), dtype=np.uint64)
    k = min(m, n)
    eye = np.zeros((m, n), dtype=np.uint8)
    eye[np.arange(k), np.arange(k)] = 1
    yield g.bits_to_words(eye)
    yield g.bits_to_words(eye[::-1].copy())
    base = g.random_words(max(m // 3, 1), n, 11)
    yield np.ascontiguousarray(np.vstack([base] * 4)[:m])
    lz = g.words_to_bits(low_rank(m, n, min(m, n) // 3, 12), n)
    lz[:, :min(n, 70)] = 0
    yield g.bits_to_words(lz)
    yield np.ascontiguousarray(np.repeat(g.random_words(1, n, 13), m, axis=0))
    one = np.zeros((m, n), dtype=np.uint8)
    one[:, n // 2] = np.arange(m) % 3 == 1
    yield g.bits_to_words(one)
