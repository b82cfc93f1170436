"""The yardstick of the weight-filtered join (include/m4ri_hip_join_select.h): the join of tests/join_ref.py followed by a numpy filter
on its weights.  It uses nothing of the library; tests/test_join_select_reference.py checks it against the definition, a loop over all
pairs.

    select(A, B, ncols, c0, b, wc0, wc1, wlo, whi, limit=None)
        -> Select(count, hits, ia, ib, D, wt): count the pairs of the join, hits those among them with wlo <= wt <= whi (wt: the ones of
           A[ia] ^ B[ib] in the columns [wc0, wc1)), and the first `limit` hits (None: all) in the join's order
"""
import collections

import numpy as np

import join_ref as jr

Select = collections.namedtuple("Select", "count hits ia ib D wt")


def select(A, B, ncols, c0, b, wc0, wc1, wlo, whi, limit=None):
    j = jr.join(A, B, ncols, c0, b, wc0, wc1)
    at = np.flatnonzero((j.wt >= wlo) & (j.wt <= whi))
    hits = len(at)
    if limit is not None:
        at = at[:limit]
    return Select(j.count, hits, j.ia[at], j.ib[at], j.D[at], j.wt[at])
