"""The yardstick of the grouping by class and of the join on a column range of any width (include/m4ri_hip_join_rows.h), from the
definition, in numpy.  It uses nothing of the library; tests/test_join_rows_reference.py checks it against a plain double loop.

A dictionary from the bits of the range of a row (unique_ref.range_words: the range in words of its own, everything else gone) to the
rows that hold them, in ascending order; the join walks the rows of A in order and, for each, the list of its value in B."""
import collections

import numpy as np

import unique_ref as ur

Join = collections.namedtuple("Join", "count ia ib d wt")


def classes(words, c0, c1):
    """-> the dictionary value -> ascending list of rows (insertion order: by lowest row), and the list of every row's key"""
    members, keys = {}, []
    for j, row in enumerate(ur.range_words(words, c0, c1)):
        key = row.tobytes()
        keys.append(key)
        members.setdefault(key, []).append(j)
    return members, keys


def group_rows(words, c0, c1):
    """-> (order, head), int32 each: the rows ascending by (lowest equal row, row); head[s] = the first position of the class of s"""
    members, _ = classes(words, c0, c1)
    order, head = [], []
    for rows in members.values():                       # a dict keeps insertion order: the classes by their lowest row
        head += [len(order)] * len(rows)
        order += rows
    return np.array(order, dtype=np.int32), np.array(head, dtype=np.int32)


def weights(words, ncols, wc0, wc1):
    """the ones of every row in the columns [wc0, wc1)"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :ncols] if len(words) else \
        np.zeros((0, ncols), dtype=np.uint8)
    return bits[:, wc0:wc1].sum(axis=1).astype(np.int32)


def join_rows(a_words, b_words, ncols, c0, c1, wc0=0, wc1=None, cap=None):
    """-> (count, ia, ib, d, wt): all pairs (i, j) with equal values, by (i, j) ascending; of them the first `cap` (None: all) with
    their XOR -- the excess bits of the last word zero -- and its ones in [wc0, wc1).  count is the number of ALL pairs"""
    wc1 = ncols if wc1 is None else wc1
    members, _ = classes(b_words, c0, c1)
    sizes = {key: len(rows) for key, rows in members.items()}
    _, keys_a = classes(a_words, c0, c1)
    count = sum(sizes.get(key, 0) for key in keys_a)
    limit = count if cap is None else min(cap, count)
    ia, ib = [], []
    for i, key in enumerate(keys_a):
        if len(ia) >= limit:
            break
        rows = members.get(key, [])[:limit - len(ia)]
        ia += [i] * len(rows)
        ib += rows
    ia, ib = np.array(ia, dtype=np.int32), np.array(ib, dtype=np.int32)
    width = (ncols + 63) // 64
    a = np.asarray(a_words, dtype=np.uint64).reshape(len(a_words), width)
    b = np.asarray(b_words, dtype=np.uint64).reshape(len(b_words), width)
    d = a[ia] ^ b[ib]
    if ncols % 64 and len(d):
        d[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    return Join(count, ia, ib, d, weights(d, ncols, wc0, wc1))
