"""The yardstick of the LF1 tests (include/m4ri_hip_bkw.h): one round of a BKW reduction in numpy on packed words.  It uses nothing of
the library; tests/test_lf1_reference.py checks it against the definition, a quadratic loop over bits.

    keys(words, c0, b)                      key(i) = bits [c0, c0 + b) of row i, bit j of the key = column c0 + j
    class_first(words, c0, b)               first[v] = the lowest i with key(i) == v, -1 for an empty class (int32[2^b])
    lf1(words, ncols, c0, b, keep_zero)     -> Lf1(first, src, partner, D): the survivors src (ascending), the row XORed into each
                                               (-1: none, a kept row of key 0), D = words[src] ^ words[partner]
"""
import collections

import numpy as np

Lf1 = collections.namedtuple("Lf1", "first src partner D")


def keys(words, c0, b):
    n = words.shape[0]
    if b == 0:
        return np.zeros(n, dtype=np.int64)
    w0, s = c0 >> 6, c0 & 63
    x = words[:, w0] >> np.uint64(s)
    if s + b > 64:
        x = x | (words[:, w0 + 1] << np.uint64(64 - s))
    return (x & np.uint64((1 << b) - 1)).astype(np.int64)


def first_of(k, b):
    first = np.full(1 << b, -1, dtype=np.int32)
    values, where = np.unique(k, return_index=True)   # return_index: the FIRST occurrence of every value
    first[values] = where
    return first


def class_first(words, c0, b):
    return first_of(keys(words, c0, b), b)


def lf1(words, ncols, c0, b, keep_zero=False):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    n = words.shape[0]
    k = keys(words, c0, b)
    first = first_of(k, b)
    rep = first[k].astype(np.int64)                   # the representative of every row's class
    own = rep == np.arange(n)
    kept = (k == 0) if keep_zero else np.zeros(n, dtype=bool)
    src = np.flatnonzero(~own | kept)
    partner = np.where(kept[src], -1, rep[src])
    D = words[src].copy()
    mixed = partner >= 0
    D[mixed] ^= words[partner[mixed]]
    if ncols % 64 and D.shape[1]:
        D[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    return Lf1(first, src.astype(np.int32), partner.astype(np.int32), D)
