"""The yardstick of the join tests (include/m4ri_hip_join.h): the join of two pools on a window of bits and the weights of the XORs, in
numpy on packed words.  It uses nothing of the library; tests/test_join_reference.py checks it against the definition, a loop over all
pairs.

    keys(words, c0, b)                       lf2_ref.keys: bit j of the key = column c0 + j
    pair_count(ka, kb)                       the sum over the keys of nA(key) * nB(key), as a Python int
    pairs(ka, kb, limit)                     -> (ia, ib) of the first `limit` outputs: for s = 0, 1, ... in the stable sorted order of
                                                A and p = l(s), ..., u(s) - 1 (the positions of B's stable sorted order with the key of s)
                                                the rows orderA[s], orderB[p]
    weights(D, wc0, wc1)                     the ones of every row of D in the columns [wc0, wc1)
    join(A, B, ncols, c0, b, wc0, wc1)       -> Join(count, ia, ib, D, wt): D[t] = A[ia[t]] ^ B[ib[t]]
"""
import collections

import numpy as np

from lf2_ref import keys, sort_keys

Join = collections.namedtuple("Join", "count ia ib D wt")


def pair_count(ka, kb):
    va, na = np.unique(ka, return_counts=True)
    vb, nb = np.unique(kb, return_counts=True)
    both, at_a, at_b = np.intersect1d(va, vb, assume_unique=True, return_indices=True)
    return int((na[at_a].astype(object) * nb[at_b].astype(object)).sum()) if len(both) else 0


def pairs(ka, kb, limit=None):
    """(ia, ib) of the first `limit` outputs (None: all)"""
    order_a, sa = sort_keys(ka)
    order_b, sb = sort_keys(kb)
    if len(sa) == 0 or len(sb) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    l = np.searchsorted(sb, sa, side="left").astype(np.int64)
    c = np.searchsorted(sb, sa, side="right").astype(np.int64) - l
    pos = np.arange(len(sa), dtype=np.int64)
    if limit is not None:                                  # the positions that hold the first `limit` outputs
        upto = int(np.searchsorted(np.cumsum(c), limit, side="left")) + 1
        pos, l, c = pos[:upto], l[:upto], c[:upto]
    before = np.cumsum(c) - c
    s = np.repeat(pos, c)
    p = np.repeat(l, c) + (np.arange(int(c.sum()), dtype=np.int64) - np.repeat(before, c))
    if limit is not None:
        s, p = s[:limit], p[:limit]
    return order_a[s], order_b[p]


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def weights(D, wc0, wc1):
    """the ones of every row of D (packed words) in the columns [wc0, wc1), int32"""
    D = np.ascontiguousarray(D, dtype=np.uint64)
    out = np.zeros(D.shape[0], dtype=np.int32)
    if wc0 >= wc1 or D.shape[0] == 0:
        return out
    for k in range(wc0 >> 6, ((wc1 - 1) >> 6) + 1):
        lo, hi = max(wc0 - 64 * k, 0), min(wc1 - 64 * k, 64)
        mask = ((1 << hi) - 1) & ~((1 << lo) - 1)
        x = np.ascontiguousarray(D[:, k] & np.uint64(mask))
        out += _POP8[x.view(np.uint8).reshape(-1, 8)].sum(axis=1, dtype=np.int32)
    return out


def join(A, B, ncols, c0, b, wc0=0, wc1=None, limit=None):
    A = np.ascontiguousarray(A, dtype=np.uint64)
    B = np.ascontiguousarray(B, dtype=np.uint64)
    ka, kb = keys(A, c0, b), keys(B, c0, b)
    ia, ib = pairs(ka, kb, limit)
    D = A[ia] ^ B[ib]
    if ncols % 64 and D.shape[1]:
        D[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    return Join(pair_count(ka, kb), ia, ib, D, weights(D, wc0, ncols if wc1 is None else wc1))
