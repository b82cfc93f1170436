"""The yardstick of the row sort on a column range and of the duplicate removal (include/m4ri_hip_unique.h), from the definition, in
numpy.  It uses nothing of the library; tests/test_unique_reference.py checks it against a second definition, Python's sorted() on big
integers.

value(i) = the integer whose bit j is column c0 + j of row i.  range_words() extracts the range into words of its own, shifted so that
column c0 is bit 0 of word 0, the top word masked: whatever the rest of a row holds -- other columns, the excess bits of the last word
-- is gone before anything is compared."""
import collections

import numpy as np

Result = collections.namedtuple("Result", "order head keep count rep")


def range_words(words, c0, c1):
    """(n, width) uint64 -> (n, ceil((c1 - c0) / 64)) uint64: the columns [c0, c1) of every row, column c0 in bit 0"""
    words = np.asarray(words, dtype=np.uint64)
    n, nbits = words.shape[0], c1 - c0
    nw = (nbits + 63) // 64
    out = np.zeros((n, nw), dtype=np.uint64)
    w0, s = c0 // 64, c0 % 64
    for k in range(nw):
        out[:, k] = words[:, w0 + k] >> np.uint64(s)
        if s and w0 + k + 1 < words.shape[1] and 64 * (k + 1) - s < nbits:       # the rest of the word comes from the next one
            out[:, k] |= words[:, w0 + k + 1] << np.uint64(64 - s)
    if nbits % 64:
        out[:, -1] &= np.uint64((1 << (nbits % 64)) - 1)
    return out


def sort_rows(words, c0, c1):
    """-> (order, head), int32 each: the rows ascending by (value, row index); head[s] = the first sorted position of the class of s"""
    n = len(words)
    v = range_words(words, c0, c1)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    # lexsort: the LAST key is the primary one, and the sort is stable: ties keep the order of the row indices
    order = np.lexsort([v[:, k] for k in range(v.shape[1])]) if v.shape[1] else np.arange(n)
    s = v[order]
    first = np.ones(n, dtype=bool)
    first[1:] = (s[1:] != s[:-1]).any(axis=1)                                     # heads by adjacent comparison
    head = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    return order.astype(np.int32), head.astype(np.int32)


def unique_rows(words, c0, c1):
    """-> (keep, count, rep): the first occurrence of every distinct value, ascending; how many; rep[i] = the lowest row equal to row i"""
    v = range_words(words, c0, c1)
    seen = {}
    rep = np.zeros(len(words), dtype=np.int32)
    for i, row in enumerate(v):
        rep[i] = seen.setdefault(row.tobytes(), i)
    keep = np.flatnonzero(rep == np.arange(len(words))).astype(np.int32)
    return keep, len(keep), rep


def everything(words, c0, c1):
    order, head = sort_rows(words, c0, c1)
    keep, count, rep = unique_rows(words, c0, c1)
    return Result(order, head, keep, count, rep)
