"""The yardstick of the subset-sum tests (include/m4ri_hip_sums.h): all XORs of p rows of a matrix in colexicographic order, with the
subsets and the weights of the sums, in numpy on packed words.  It uses nothing of the library; tests/test_sums_reference.py checks it
against the definition, itertools.combinations sorted by the reversed tuple.

    count(n, p)                              C(n, p), a Python int
    rank(c)                                  C(c_1, 1) + ... + C(c_p, p) of an ascending tuple, a Python int
    unrank(r, p)                             the ascending tuple of that rank (exact integer arithmetic, any size)
    successor(c)                             the tuple of the next rank
    all_subsets(n, p)                        every subset of {0 .. n - 1} of size p, by itertools, sorted by rank: (C(n, p), p) int32
    subsets(n, p, rank0, count)              the subsets of the ranks [rank0, rank0 + count): a slice of all_subsets where that is
                                             small, else unrank(rank0) and count - 1 successors
    sums(S, ncols, p, base, rank0, count, wc0, wc1)   -> Sums(D, idx, wt): D[t] = base ^ S[c_1] ^ ... ^ S[c_p], idx[t] = (c_1 .. c_p),
                                             wt[t] = the ones of D[t] in the columns [wc0, wc1)
"""
import collections
import functools
import itertools
import math

import numpy as np

from join_ref import weights

Sums = collections.namedtuple("Sums", "D idx wt")
ENUMERATE_UP_TO = 300000        # subsets that all_subsets may make


def count(n, p):
    return math.comb(n, p) if n >= p else 0


def rank(c):
    assert c[0] >= 0 and all(a < b for a, b in zip(c, c[1:])), c
    return sum(math.comb(int(ci), i + 1) for i, ci in enumerate(c))


def unrank(r, p):
    c = [0] * p
    for i in range(p, 0, -1):
        lo, hi = i - 1, i        # C(lo, i) = 0 <= r; find a hi with C(hi, i) > r, then bisect
        while math.comb(hi, i) <= r:
            hi *= 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if math.comb(mid, i) <= r:
                lo = mid
            else:
                hi = mid
        c[i - 1] = lo
        r -= math.comb(lo, i)
    assert r == 0
    return tuple(c)


def successor(c):
    c = list(c)
    for i in range(len(c)):
        if i + 1 == len(c) or c[i] + 1 < c[i + 1]:
            c[i] += 1
            return tuple(c)
        c[i] = i                 # back to the smallest value of this level; the carry goes up
    raise AssertionError


@functools.lru_cache(maxsize=64)
def all_subsets(n, p):
    assert count(n, p) <= ENUMERATE_UP_TO
    rows = sorted(itertools.combinations(range(n), p), key=lambda c: c[::-1])
    out = np.array(rows, dtype=np.int32).reshape(len(rows), p)
    out.setflags(write=False)
    return out


def subsets(n, p, rank0=0, cnt=None):
    total = count(n, p)
    cnt = total - rank0 if cnt is None else cnt
    assert 0 <= rank0 and cnt >= 0 and rank0 + cnt <= total, (n, p, rank0, cnt)
    if total <= ENUMERATE_UP_TO:
        return all_subsets(n, p)[rank0:rank0 + cnt].copy()
    out = np.zeros((cnt, p), dtype=np.int32)
    c = unrank(rank0, p) if cnt else None
    for t in range(cnt):
        out[t] = c
        c = successor(c)
    return out


def sums(S, ncols, p, base=None, rank0=0, cnt=None, wc0=0, wc1=None):
    S = np.ascontiguousarray(S, dtype=np.uint64)
    n, nw = S.shape[0], (ncols + 63) // 64
    idx = subsets(n, p, rank0, cnt)
    D = np.zeros((len(idx), nw), dtype=np.uint64)
    if base is not None:
        D ^= np.asarray(base, dtype=np.uint64).reshape(1, nw)
    for i in range(p):
        D ^= S[idx[:, i], :nw]
    if ncols % 64 and nw:
        D[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    return Sums(D, idx, weights(D, wc0, ncols if wc1 is None else wc1))
