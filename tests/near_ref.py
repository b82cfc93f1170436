"""The yardstick of the Hamming-distance search (include/m4ri_hip_near.h), from the definition, in numpy.  It uses nothing of the library;
tests/test_near_reference.py checks it against a plain double loop.

    distances(A, B, ncols, wc0, wc1)            -> the NA x NB table d(i, j): the ones of A[i] ^ B[j] in the columns [wc0, wc1)  (int64)
    admitted(NA, NB, flags)                     -> the NA x NB table of the pairs that the flags admit  (bool)
    near_pairs(A, B, ncols, wc0, wc1, wlo, whi, flags=0, limit=None)
        -> Pairs(hits, ia, ib, D, wt): hits the number of admitted pairs with wlo <= d <= whi, and the first `limit` of them (None: all)
           in the order (ia, ib)
    nearest(A, B, ncols, wc0, wc1, flags=0)     -> (idx, dist): the lowest nearest admitted row of B for every row of A; -1, -1: none

A and B are uint64 words, NA x width(ncols) and NB x width(ncols).  The tables are built in slabs of rows of A, so that pools of a few
ten thousand rows stay affordable."""
import collections

import numpy as np

OFF_DIAGONAL, UPPER = 1, 2
Pairs = collections.namedtuple("Pairs", "hits ia ib D wt")

_BYTE_ONES = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)


def _range_masks(ncols, wc0, wc1):
    """per word of a row: the bits that are columns of [wc0, wc1)"""
    nw = (ncols + 63) // 64
    masks = np.zeros(nw, dtype=np.uint64)
    for k in range(nw):
        lo, hi = max(wc0, 64 * k), min(wc1, 64 * k + 64)
        if lo < hi:
            masks[k] = np.uint64(((1 << (hi - lo)) - 1) << (lo - 64 * k))
    return masks


def distances(A, B, ncols, wc0, wc1):
    NA, NB = len(A), len(B)
    out = np.zeros((NA, NB), dtype=np.int64)
    masks = _range_masks(ncols, wc0, wc1)
    for k in np.flatnonzero(masks):
        x = (A[:, k, None] ^ B[None, :, k]) & masks[k]
        out += _BYTE_ONES[np.ascontiguousarray(x).view(np.uint8).reshape(NA, NB, 8)].sum(axis=2, dtype=np.int64)
    return out


def admitted(NA, NB, flags, i0=0):
    """the rows i0 .. i0 + NA of A against all rows of B"""
    i, j = np.arange(i0, i0 + NA)[:, None], np.arange(NB)[None, :]
    if flags & UPPER:
        return i < j
    if flags & OFF_DIAGONAL:
        return i != j
    return np.ones((NA, NB), dtype=bool)


def _slabs(NA, NB):
    step = max(1, (1 << 22) // max(NB, 1))
    return [(i0, min(i0 + step, NA)) for i0 in range(0, NA, step)]


def near_pairs(A, B, ncols, wc0, wc1, wlo, whi, flags=0, limit=None):
    nw = (ncols + 63) // 64
    hits, ia, ib, wt = 0, [], [], []
    for i0, i1 in _slabs(len(A), len(B)):
        d = distances(A[i0:i1], B, ncols, wc0, wc1)
        hit = (d >= wlo) & (d <= whi) & admitted(i1 - i0, len(B), flags, i0)
        hits += int(hit.sum())
        i, j = np.nonzero(hit)                       # row-major: ascending i, then ascending j
        ia.append(i + i0)
        ib.append(j)
        wt.append(d[i, j])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)  # noqa: E731
    ia, ib, wt = cat(ia)[:limit], cat(ib)[:limit], cat(wt)[:limit]
    D = (A[ia] ^ B[ib]) if len(ia) else np.zeros((0, nw), dtype=np.uint64)
    return Pairs(hits, ia.astype(np.int32), ib.astype(np.int32), D, wt.astype(np.int32))


def nearest(A, B, ncols, wc0, wc1, flags=0):
    NA, NB = len(A), len(B)
    idx, dist = np.full(NA, -1, dtype=np.int32), np.full(NA, -1, dtype=np.int32)
    if NB == 0:
        return idx, dist
    far = np.iinfo(np.int64).max
    for i0, i1 in _slabs(NA, NB):
        d = np.where(admitted(i1 - i0, NB, flags, i0), distances(A[i0:i1], B, ncols, wc0, wc1), far)
        j = d.argmin(axis=1)                        # the first of equals: the lowest row
        best = d[np.arange(i1 - i0), j]
        some = best != far
        idx[i0:i1][some] = j[some]
        dist[i0:i1][some] = best[some]
    return idx, dist
