"""tests/cover_ref.py against the definitions, without the library: the coset leaders against the full enumeration of all 2^n patterns,
the named codes against what include/m4ri_hip_cover.h pins, and the row-wise reduction against a loop over bits."""
import numpy as np
import pytest

import cover_ref as cr
import gf2util as g


def random_systematic(n, k, seed):
    rng = np.random.default_rng(seed)
    return cr.Code(n, k, tuple(int(rng.integers(0, 1 << k)) | 1 << (k + t) for t in range(n - k)))


def parity(x):
    return bin(x).count("1") & 1


def leaders_by_enumeration(code):
    r = code.n - code.k
    best = {}
    for e in range(1 << code.n):                      # ascending: among equal weights the first one met is the smallest
        s = sum(parity(e & code.h[t]) << t for t in range(r))
        w = bin(e).count("1")
        if s not in best or w < best[s][0]:
            best[s] = (w, e)
    assert len(best) == 1 << r
    return np.array([best[s][1] for s in range(1 << r)], dtype=np.uint32), max(w for w, _ in best.values())


SMALL = [cr.repetition(3), cr.repetition(5), cr.repetition(6), cr.hamming(3), cr.hamming(4), random_systematic(12, 6, 5)]


@pytest.mark.parametrize("code", SMALL, ids=lambda c: "%d-%d" % (c.n, c.k))
def test_leaders_are_the_enumeration(code):
    want, radius = leaders_by_enumeration(code)
    got, got_radius = cr.leaders(code)
    assert got.dtype == np.uint32 and np.array_equal(got, want) and got_radius == radius
    assert np.array_equal(cr.syndromes(code, got), np.arange(1 << (code.n - code.k)))


def test_ties_go_to_the_smaller_integer():
    table, radius = cr.leaders(cr.repetition(6))       # weight 3 on either side: 0b000111 wins over 0b111000
    assert radius == 3 and 0b000111 in table and 0b111000 not in table
    assert sorted(cr.popcount(table)) == sorted([0] + [1] * 6 + [2] * 15 + [3] * 10)


def test_the_named_codes():
    assert cr.hamming(3) == cr.Code(7, 4, (0b0011011, 0b0101101, 0b1001110))    # columns 3, 5, 6, 7 and the identity
    assert cr.repetition(3) == cr.Code(3, 1, (0b011, 0b101))
    for code in [cr.hamming(r) for r in range(2, 6)] + [cr.repetition(n) for n in range(2, 14)] + [cr.golay23()]:
        r = code.n - code.k
        assert len(code.h) == r <= cr.MAX_R and all(code.h[t] >> code.k == 1 << t for t in range(r))
    for r in range(2, 6):                                # perfect, radius 1: the leaders are 0 and the n unit patterns
        table, radius = cr.leaders(cr.hamming(r))
        assert radius == 1 and sorted(table) == [0] + [1 << j for j in range((1 << r) - 1)]
    for n in range(2, 14):
        assert cr.leaders(cr.repetition(n))[1] == n // 2
    assert list(cr.leaders(cr.identity(9))[0]) == [0] and cr.leaders(cr.identity(9))[1] == 0 and len(cr.leaders(cr.drop(9))[0]) == 0


def test_golay():
    code = cr.golay23()
    table, radius = cr.leaders(code)
    assert radius == 3 and list(np.bincount(cr.popcount(table))) == [1, 23, 253, 1771]      # perfect
    # g divides every codeword: the code is the cyclic one
    words = cr.encode(code, np.arange(1 << 12))
    assert not cr.syndromes(code, words).any()
    assert min(bin(int(w)).count("1") for w in words[1:]) == 7
    # message u sits in the low bits, the checks above: the polynomial is x^11 u(x) + (x^11 u(x) mod g) read from the top
    g23, u = 0b110001110101, 0b101100000001
    rem = u << 11
    for d in range(22, 10, -1):
        if rem >> d & 1:
            rem ^= g23 << (d - 11)
    assert int(words[u]) == u | rem << 12


def reduce_by_bits(bits, c0, segments, tables):
    N = bits.shape[0]
    out, dist = [[] for _ in range(N)], [0] * N
    o = c0
    for j, code in enumerate(segments):
        r = code.n - code.k
        table = tables[j] if tables and tables[j] is not None else cr.leaders(code)[0]
        for i in range(N):
            a = sum(int(bits[i, o + t]) << t for t in range(code.n))
            if r == 0:
                e = 0
            elif code.k == 0:
                e = a
            else:
                e = int(table[sum(parity(a & code.h[t]) << t for t in range(r))]) & cr.mask(code.n)
            dist[i] += bin(e).count("1")
            out[i] += [((a ^ e) >> t) & 1 for t in range(code.k)]
        o += code.n
    return np.array(out, dtype=np.uint8).reshape(N, sum(c.k for c in segments)), np.array(dist)


LIST = [cr.golay23(), cr.hamming(3), cr.repetition(3), cr.identity(1), cr.drop(12), cr.hamming(5), cr.repetition(13), cr.identity(32),
        cr.hamming(4)]


@pytest.mark.parametrize("case", [(0, LIST), (37, LIST), (63, LIST[::-1]), (64, LIST[::-1]), (5, [cr.identity(32)] * 4 + [cr.drop(3)]),
                                  (33, [cr.identity(32)]), (0, [cr.drop(7), cr.drop(32)]), (9, [])], ids=lambda c: "c%d-%d" % (c[0], len(c[1])))
def test_reduce_is_the_loop_over_bits(case):
    c0, segments = case
    ncols = c0 + sum(c.n for c in segments) + 11
    rng = np.random.default_rng(c0)
    bits = rng.integers(0, 2, (60, ncols), dtype=np.uint8)
    tables = None
    if c0 == 37:     # a table that is no leader table is taken as it is
        tables = [rng.integers(0, 1 << 32, 1 << (c.n - c.k), dtype=np.uint32) if cr.has_table(c) and j % 2 else None for j, c in enumerate(segments)]
    D, dist = cr.reduce(g.bits_to_words(bits), c0, segments, tables)
    want, want_dist = reduce_by_bits(bits, c0, segments, tables)
    K = want.shape[1]
    assert D.dtype == np.uint64 and D.shape == (60, g.width(K)) and dist.dtype == np.int32
    assert np.array_equal(dist, want_dist)
    if K:
        assert np.array_equal(g.words_to_bits(D, K), want)
        assert K % 64 == 0 or not (D[:, -1] >> np.uint64(K % 64)).any()
    if tables is None and K:
        # with leader tables: the re-encoded messages lie dist away from the blocks, and no codeword is nearer than the radius says
        o = q = 0
        away = np.zeros(60, dtype=np.int64)
        for code in segments:
            a = cr.blocks(g.bits_to_words(bits), c0 + o, code.n)
            m = cr.blocks(D, q, code.k) if code.k else np.zeros(60, dtype=np.uint64)
            away += cr.popcount(a ^ cr.encode(code, m)) if code.k else cr.popcount(a)
            o, q = o + code.n, q + code.k
        assert np.array_equal(away, dist) and dist.max() <= sum(cr.leaders(c)[1] if c.k else c.n for c in segments)
