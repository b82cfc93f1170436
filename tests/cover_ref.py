"""The yardstick of the covering-code tests (include/m4ri_hip_cover.h) in numpy on packed words.  It uses nothing of the library;
tests/test_cover_reference.py checks it against full enumeration and a loop over bits.

    Code(n, k, h)                            an [n, k] code: bit t of the syndrome of a block a is parity(a & h[t]), h[t] >> k == 1 << t
    identity(n) drop(n) repetition(n) hamming(r) golay23()     the named codes, as the header pins them
    syndromes(code, a)                       the syndrome of every block of the uint32 array a
    leaders(code) -> (uint32[2^r], radius)   leaders[s] = the pattern of LOWEST weight with syndrome s, among equal weights the smallest
                                             integer; for k == 0: no entry, for r == 0: [0]
    encode(code, u)                          the codeword (u, A u) of every message of the array u
    reduce(words, c0, segments, tables=None) -> (D words, dist int32): block j of every row decoded by segments[j]; tables[j] (None:
                                             the leaders) is read as it is
"""
import collections
import functools
import itertools

import numpy as np

Code = collections.namedtuple("Code", "n k h")
MAX_R = 12
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popcount(a):
    a = np.asarray(a, dtype=np.uint64)
    return sum(_POP8[((a >> np.uint64(8 * i)) & np.uint64(255)).astype(np.int64)] for i in range(8))


def mask(n):
    return (1 << n) - 1


def identity(n):
    return Code(n, n, ())


def drop(n):
    return Code(n, 0, ())


def repetition(n):
    return Code(n, 1, tuple(1 | 1 << (1 + t) for t in range(n - 1)))


def hamming(r):
    n = (1 << r) - 1
    k = n - r
    cols = [v for v in range(1, 1 << r) if v & (v - 1)]      # not a power of two, ascending
    return Code(n, k, tuple(sum(((v >> t) & 1) << j for j, v in enumerate(cols)) | 1 << (k + t) for t in range(r)))


def golay23():
    g, cols = 0b110001110101, []                              # x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1
    for i in range(12):
        rem = 1 << (11 + i)
        for d in range(11 + i, 10, -1):
            if rem >> d & 1:
                rem ^= g << (d - 11)
        cols.append(rem)
    return Code(23, 12, tuple(sum(((c >> t) & 1) << i for i, c in enumerate(cols)) | 1 << (12 + t) for t in range(11)))


def has_table(code):
    return 0 < code.k < code.n


def syndromes(code, a):
    a = np.asarray(a, dtype=np.uint64)
    s = np.zeros(a.shape, dtype=np.int64)
    for t in range(code.n - code.k):
        s |= (popcount(a & np.uint64(code.h[t])) & 1) << t
    return s


@functools.lru_cache(maxsize=None)
def _leaders(code):
    r = code.n - code.k
    if code.k == 0:
        return np.zeros(0, dtype=np.uint32), 0
    out = np.zeros(1 << r, dtype=np.uint32)
    seen = np.zeros(1 << r, dtype=bool)
    seen[0] = True
    w = 0
    while not seen.all():
        w += 1
        # every pattern of weight w, ascending as integers: the first one met with a new syndrome is that syndrome's leader
        pats = np.sort(np.array([sum(1 << j for j in c) for c in itertools.combinations(range(code.n), w)], dtype=np.uint64))
        syn = syndromes(code, pats)
        first = np.unique(syn, return_index=True)             # return_index: the FIRST occurrence of every value
        for s, at in zip(*first):
            if not seen[s]:
                seen[s] = True
                out[s] = pats[at]
    return out, w


def leaders(code):
    table, radius = _leaders(code)
    return table.copy(), radius


def encode(code, u):
    u = np.asarray(u, dtype=np.uint64) & np.uint64(mask(code.k))
    if code.k == code.n or code.k == 0:
        return u
    return u | (syndromes(Code(code.n, code.k, tuple(x & mask(code.k) for x in code.h)), u).astype(np.uint64) << np.uint64(code.k))


def blocks(words, o, n):
    """bits [o, o + n) of every row, n <= 32"""
    w0, s = o >> 6, o & 63
    x = words[:, w0] >> np.uint64(s)
    if s + n > 64:
        x = x | (words[:, w0 + 1] << np.uint64(64 - s))
    return x & np.uint64(mask(n))


def reduce(words, c0, segments, tables=None):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    N = words.shape[0]
    K = sum(c.k for c in segments)
    D = np.zeros((N, (K + 63) // 64), dtype=np.uint64)
    dist = np.zeros(N, dtype=np.int64)
    o, q = c0, 0
    for j, code in enumerate(segments):
        a = blocks(words, o, code.n) if N else np.zeros(0, dtype=np.uint64)
        if code.k == code.n:
            e = np.zeros(N, dtype=np.uint64)
        elif code.k == 0:
            e = a
        else:
            table = leaders(code)[0] if tables is None or tables[j] is None else np.asarray(tables[j], dtype=np.uint32)
            e = table[syndromes(code, a)].astype(np.uint64) & np.uint64(mask(code.n))
        dist += popcount(e)
        m = (a ^ e) & np.uint64(mask(code.k))
        if code.k:
            D[:, q >> 6] |= m << np.uint64(q & 63)
            if (q & 63) + code.k > 64:
                D[:, (q >> 6) + 1] |= m >> np.uint64(64 - (q & 63))
        o += code.n
        q += code.k
    return D, dist.astype(np.int32)
