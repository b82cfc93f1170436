"""The yardstick of the LF2 tests (include/m4ri_hip_lf2.h): the stable class sort and one LF2 round in numpy on packed words.  It uses
nothing of the library; tests/test_lf2_reference.py checks it against the definition, a loop over classes and pairs.

    keys(words, c0, b)             key(i) = bits [c0, c0 + b) of row i, bit j of the key = column c0 + j
    class_sort(words, c0, b)       -> (order, skeys): argsort(kind="stable") of the keys, and the keys in that order
    pairs(k)                       -> (lo, hi) of the keys k: for s = 0, 1, ... in sorted order and p = t(s), ..., s - 1 (t(s): the first
                                      position of the class of s) the rows order[p], order[s]
    lf2(words, ncols, c0, b)       -> Lf2(count, lo, hi, D): D[j] = words[hi[j]] ^ words[lo[j]]
"""
import collections

import numpy as np

Lf2 = collections.namedtuple("Lf2", "count lo hi D")


def keys(words, c0, b):
    n = words.shape[0]
    if b == 0:
        return np.zeros(n, dtype=np.int64)
    w0, s = c0 >> 6, c0 & 63
    x = words[:, w0] >> np.uint64(s)
    if s + b > 64:
        x = x | (words[:, w0 + 1] << np.uint64(64 - s))
    return (x & np.uint64((1 << b) - 1)).astype(np.int64)


def sort_keys(k):
    order = np.argsort(k, kind="stable")
    return order.astype(np.int32), np.asarray(k)[order].astype(np.int32)


def class_sort(words, c0, b):
    return sort_keys(keys(words, c0, b))


def pair_count(k):
    """the sum over the classes of n (n - 1) / 2, as a Python int"""
    sizes = np.unique(k, return_counts=True)[1].astype(object)
    return int((sizes * (sizes - 1) // 2).sum()) if len(sizes) else 0


def pairs(k, limit=None):
    """(lo, hi) of the first `limit` outputs (None: all)"""
    order, sk = sort_keys(k)
    n = len(sk)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    pos = np.arange(n, dtype=np.int64)
    head = np.ones(n, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    t = np.maximum.accumulate(np.where(head, pos, 0))      # the first position of every position's class
    r = pos - t                                            # outputs of position s
    if limit is not None:                                  # the positions that hold the first `limit` outputs
        upto = int(np.searchsorted(np.cumsum(r), limit, side="left")) + 1
        pos, t, r = pos[:upto], t[:upto], r[:upto]
    before = np.cumsum(r) - r
    s = np.repeat(pos, r)
    p = np.repeat(t, r) + (np.arange(int(r.sum()), dtype=np.int64) - np.repeat(before, r))
    if limit is not None:
        s, p = s[:limit], p[:limit]
    return order[p], order[s]


def lf2(words, ncols, c0, b, limit=None):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    k = keys(words, c0, b)
    lo, hi = pairs(k, limit)
    D = words[hi] ^ words[lo]
    if ncols % 64 and D.shape[1]:
        D[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    return Lf2(pair_count(k), lo, hi, D)
