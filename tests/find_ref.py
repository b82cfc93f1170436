"""The yardstick of the row lookup (include/m4ri_hip_find.h), from the definition, in numpy.  It uses nothing of the library;
tests/test_find_reference.py checks it against a brute-force double loop, against the yardstick of the duplicate removal and against
numpy.unique.

A dictionary from the bits of the range of a row of B (unique_ref.range_words: the range in words of its own, everything else gone)
to (the first row that holds them, how many rows hold them); every row of A is looked up in it."""
import collections

import numpy as np

import unique_ref as ur

Result = collections.namedtuple("Result", "idx mult count")


def find_rows(a_words, b_words, c0, c1):
    """-> (idx, mult, count): idx[i] the lowest row of B equal to row i of A on the columns [c0, c1), -1 for none; mult[i] the
    number of such rows; count the rows of A with idx >= 0"""
    va, vb = ur.range_words(a_words, c0, c1), ur.range_words(b_words, c0, c1)
    seen = {}
    for j, row in enumerate(vb):
        key = row.tobytes()
        first, size = seen.get(key, (j, 0))
        seen[key] = (first, size + 1)
    idx = np.full(len(va), -1, dtype=np.int32)
    mult = np.zeros(len(va), dtype=np.int32)
    for i, row in enumerate(va):
        idx[i], mult[i] = seen.get(row.tobytes(), (-1, 0))
    return Result(idx, mult, int((idx >= 0).sum()))
