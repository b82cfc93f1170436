"""GPU tests of gf2_gather_rows_dev and gf2_gather_cols_dev (include/m4ri_hip_gather.h; kernels: m4ri-rust_amd/csrc/gather) through
device.gather_rows / gather_cols / DMat.take_rows / take_cols.  Expected values come from numpy fancy indexing on unpacked bits
(gf2util.words_to_bits / bits_to_words), independent of the library.  Every case compares the WHOLE buffer its destination lives in, so
the matrix, the excess bits of its last word and every neighbouring word are checked; sources and index arrays are compared too.

Operands come in two kinds: `plain`, a buffer of its own with an even row stride on a 16-byte boundary, and `view`, an odd row stride
at an odd word inside a parent full of random bits -- for a source the excess bits of the view's last word are random too."""
import ctypes
import gc

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import limits_ref as lr
from census_util import assert_route, census
from stream_util import run_pending

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


@pytest.fixture(scope="module")
def dev(pkg):
    from m4ri_rust_amd import device
    return device


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def to_gpu(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()


def ints_to_gpu(values):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32).copy()).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def dirty(nrows, ld, seed):
    return g.splitmix64(seed, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld)


class Operand:
    """`words` (nrows x width(ncols)) on the device, as a buffer of its own or as a view of a dirty parent; .host is what the whole
    buffer holds, .at the place of the matrix in it"""

    def __init__(self, dev, words, ncols, view, seed, dirty_excess=False):
        nrows, w = words.shape
        if view:
            ld = w + 3 if (w + 3) & 1 else w + 4
            r0, c0 = 1, 2                       # word r0 * ld + c0 of the parent: odd
            self.host = dirty(nrows + 3, ld, seed)
        else:
            ld = (w + 1) & ~1
            r0, c0 = 0, 0
            self.host = dirty(max(nrows, 1), ld, seed)[:nrows]
        words = words.copy()
        if dirty_excess and ncols % 64:
            words[:, -1] |= dirty(nrows, 1, seed + 1)[:, 0] & ~np.uint64((1 << (ncols % 64)) - 1)
        self.at = (slice(r0, r0 + nrows), slice(c0, c0 + w))
        self.host[self.at] = words
        self.t = to_gpu(self.host) if self.host.size else None
        base = self.t.data_ptr() if self.t is not None else 0
        self.m = dev.DMat.wrap(base + 8 * (r0 * ld + c0) if base else 0, nrows, ncols, ld, keep=self.t)

    def now(self):
        return to_host(self.t).reshape(self.host.shape)


def gathered_bits(sbits, idx, axis, count):
    """numpy fancy indexing with -1 and everything out of range as zeros"""
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < sbits.shape[axis])
    if axis == 0:
        out = np.zeros((count, sbits.shape[1]), dtype=np.uint8)
        out[ok] = sbits[idx[ok]]
    else:
        out = np.zeros((sbits.shape[0], count), dtype=np.uint8)
        out[:, ok] = sbits[:, idx[ok]]
    return out, bool(np.any(~ok & (idx != -1)))


def run_gather(dev, axis, d_shape, s_shape, idx, accumulate=False, view=False, seed=1, stream=None):
    """one call on fresh operands with a raw device index array and a zeroed device flag; checks the destination's whole buffer, the
    source, the index array and the flag; -> the destination's words"""
    import torch
    (dn, dc), (sn, sc) = d_shape, s_shape
    s = g.random_words(sn, sc, seed) if sn and sc else np.zeros((sn, g.width(sc)), dtype=np.uint64)
    d0 = dirty(dn, g.width(dc), seed + 100)   # excess bits included: a fresh block is not cleared
    S = Operand(dev, s, sc, view, seed + 200, dirty_excess=True)
    D = Operand(dev, d0, dc, view, seed + 300)
    ti, tb = ints_to_gpu(idx), ints_to_gpu([0])
    torch.cuda.synchronize()
    if axis == 0:
        out, flag = dev.gather_rows(S.m, ti.data_ptr(), D=D.m, accumulate=accumulate, bad=tb.data_ptr(), stream=stream)
    else:
        out, flag = dev.gather_cols(S.m, ti.data_ptr(), D=D.m, bad=tb.data_ptr(), stream=stream)
    assert out is D.m and flag is None
    torch.cuda.synchronize()
    sbits = g.words_to_bits(s, sc) if sn and sc else np.zeros((sn, sc), dtype=np.uint8)
    bits, want_bad = gathered_bits(sbits, idx, axis, dn if axis == 0 else dc)
    want = g.bits_to_words(bits)
    if accumulate:
        idx64 = np.asarray(idx, dtype=np.int64)
        keep = ~((idx64 >= 0) & (idx64 < sn))
        want = d0 ^ want
        want[keep] = d0[keep]
    expect = D.host.copy()
    expect[D.at] = want
    got = D.now()
    bad_words = np.argwhere(got != expect)
    assert not len(bad_words), "%d wrong words in the destination's buffer, first at %s" % (len(bad_words), tuple(bad_words[0]))
    if S.t is not None:
        assert np.array_equal(S.now(), S.host), "the source changed"
    assert np.array_equal(ti.cpu().numpy(), np.asarray(idx, dtype=np.int32)), "the index array changed"
    assert int(tb.cpu()[0]) == int(want_bad), "bad is %d, want %d" % (int(tb.cpu()[0]), want_bad)
    return want


def patterns(count, n, seed):
    """index patterns for `count` indices into n rows / columns"""
    rng = np.random.default_rng(seed)
    return {
        "identity": np.arange(count) % max(n, 1),
        "reversed": (n - 1 - np.arange(count)) % max(n, 1),
        "one": np.full(count, n // 2),
        "none": np.full(count, -1),
        "random": rng.integers(0, max(n, 1), count),
    }


# ---- rows -----------------------------------------------------------------------------------------------------------------------------

ROW_SHAPES = [(1, 1, 1), (5, 3, 64), (300, 7, 65), (129, 1000, 191), (1000, 129, 4097)]


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_rows(dev, shape, accumulate, view):
    dn, sn, ncols = shape
    for name, idx in patterns(dn, sn, 7).items():
        run_gather(dev, 0, (dn, ncols), (sn, ncols), idx, accumulate, view, seed=11)


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_rows_bad_indices(dev, accumulate, view):
    """out-of-range values give zero rows (accumulate: untouched rows) and bad == 1 -- run_gather asserts the flag both ways; -1 alone
    leaves it 0"""
    dn, sn, ncols = 300, 7, 191
    idx = np.random.default_rng(3).integers(0, sn, dn)
    idx[[0, 5, 64, 65, 128, 299]] = [sn, INT_MIN, INT_MAX, -2, sn + 1, -1]
    run_gather(dev, 0, (dn, ncols), (sn, ncols), idx, accumulate, view, seed=21)
    only_minus_one = idx.copy()
    only_minus_one[[0, 5, 64, 65, 128, 299]] = -1
    run_gather(dev, 0, (dn, ncols), (sn, ncols), only_minus_one, accumulate, view, seed=22)
    # an empty source: D comes out zero (accumulate: unchanged), and every index but -1 counts as bad
    run_gather(dev, 0, (5, 70), (0, 70), [0, -1, 3, -1, INT_MAX], accumulate, view, seed=23)
    run_gather(dev, 0, (5, 70), (0, 70), [-1] * 5, accumulate, view, seed=24)


def test_rows_from_a_source_past_4gib(dev, L):
    """130 rows from the end of an 8 400 000 x 4096 source (4.3 GB): the row offset of the source does not fit 32 bits"""
    import torch
    sn, ncols, seed = 8_400_000, 4096, 0x6A7
    gc.collect()
    L.gf2_trim()
    S = dev.DMat.random(sn, ncols, seed)
    rng = np.random.default_rng(5)
    idx = np.concatenate([sn - 1 - rng.integers(0, 1000, 126), [sn - 1, 0, sn, 8_388_608]])   # 2^23 rows in: byte offset 2^32
    D = dev.DMat(len(idx), ncols)
    ti, tb = ints_to_gpu(idx), ints_to_gpu([0])
    dev.gather_rows(S, ti.data_ptr(), D=D, bad=tb.data_ptr())
    got = D.to_words()
    want = lr.seeded_words(seed, ncols, np.where(idx < sn, idx, 0))
    want[idx >= sn] = 0
    assert np.array_equal(got, want)
    assert int(tb.cpu()[0]) == 1
    del S, D
    gc.collect()
    L.gf2_trim()


# ---- columns --------------------------------------------------------------------------------------------------------------------------

COL_SHAPES = [(1, 1, 1), (64, 64, 64), (65, 65, 65), (63, 127, 129), (130, 200, 70), (200, 1000, 1), (100, 1, 300), (257, 4133, 4096)]


def first_composed(dev, nrows=70):
    lo, hi = 1, 1 << 24
    assert dev.gather_cols_plan(nrows, lo, 64)[0] == 0 and dev.gather_cols_plan(nrows, hi, 64)[0] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if dev.gather_cols_plan(nrows, mid, 64)[0] == 0 else (lo, mid)
    return hi


def routed(dev, L, rows, sc, dc, fn):
    """fn() under the census: the kernels the plan names are the ones that ran"""
    path = dev.gather_cols_plan(rows, sc, dc)[0]
    k0 = census(L)
    out = fn()
    k1 = census(L)
    ran = sorted(k for k, v in k1.items() if v > k0.get(k, 0))
    if path == 0:
        assert_route(k0, k1, ["gf2_gather_cols_kernel"])
        assert not [k for k in ran if "gf2_transpose" in k or "gf2_gather_rows" in k], ran
    else:
        assert_route(k0, k1, ["gf2_transpose", "gf2_gather_rows_kernel"])
        assert not [k for k in ran if "gf2_gather_cols" in k], ran
    return out


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("shape", COL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_cols_fused(dev, L, shape, view):
    rows, sc, dc = shape
    assert dev.gather_cols_plan(rows, sc, dc)[0] == 0
    for name, idx in patterns(dc, sc, 9).items():
        routed(dev, L, rows, sc, dc, lambda: run_gather(dev, 1, (rows, dc), (rows, sc), idx, False, view, seed=31))


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
def test_cols_bad_indices(dev, L, view):
    rows, sc, dc = 130, 200, 270   # D wider than S; the last band ends after two rows
    idx = np.random.default_rng(4).integers(0, sc, dc)
    idx[[0, 63, 64, 128, 200, 269]] = [sc, INT_MIN, INT_MAX, -2, sc + 56, -1]   # sc + 56 = 256: inside S's last word, outside S
    run_gather(dev, 1, (rows, dc), (rows, sc), idx, False, view, seed=41)
    idx[[0, 63, 64, 128, 200, 269]] = -1
    run_gather(dev, 1, (rows, dc), (rows, sc), idx, False, view, seed=42)
    # an empty source (no columns): a zero D, and every index but -1 counts as bad
    run_gather(dev, 1, (70, 5), (70, 0), [0, -1, 3, -1, INT_MIN], False, view, seed=43)
    run_gather(dev, 1, (70, 5), (70, 0), [-1] * 5, False, view, seed=44)


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("over", [0, 1])
def test_cols_composed(dev, L, over, view):
    """the smallest source width the plan sends through transpose / row gather / transpose, and one column more; 70 rows"""
    rows, sc = 70, first_composed(dev) + over
    assert dev.gather_cols_plan(rows, sc - 1 - over, 100)[0] == 0 and dev.gather_cols_plan(rows, sc, 100)[0] == 1
    rng = np.random.default_rng(6)
    for dc, idx in ((sc, rng.permutation(sc)), (131, np.concatenate([rng.integers(0, sc, 125), [sc - 1, 0, -1, sc, INT_MAX, -7]]))):
        routed(dev, L, rows, sc, dc, lambda: run_gather(dev, 1, (rows, dc), (rows, sc), idx, False, view, seed=51))


def test_cols_consistency(dev, L):
    rows, n = 130, 517
    rng = np.random.default_rng(8)
    s = g.random_words(rows, n, 61)
    S = dev.DMat.from_words(s, n)
    p = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[p] = np.arange(n)
    # a permutation and its inverse restore S; the wrapper uploads lists and arrays and reports the flag itself
    G, bad = dev.gather_cols(S, p, bad=None)
    assert bad is False
    back, bad = dev.gather_cols(G, list(inv), bad=None)
    assert bad is False and np.array_equal(back.to_words(), s)
    assert np.array_equal(G.to_words(), g.bits_to_words(g.words_to_bits(s, n)[:, p]))
    # columns of S are rows of its transpose
    viarows = dev.transpose(dev.gather_rows(dev.transpose(S), p)[0])
    assert np.array_equal(viarows.to_words(), G.to_words())
    assert np.array_equal(S.take_cols(p).to_words(), G.to_words())
    assert np.array_equal(S.take_rows([3, 3, -1, 129]).to_words(), g.bits_to_words(gathered_bits(g.words_to_bits(s, n), [3, 3, -1, 129], 0, 4)[0]))
    assert dev.gather_rows(S, [0, rows], bad=None)[1] is True
    # a transposition list applied to the columns by gf2_apply_p_dev(right = 1): swaps (i, P[i]), i descending
    P = [int(rng.integers(i, n)) for i in range(n)]
    cols = np.arange(n)
    for i in reversed(range(n)):
        cols[[i, P[i]]] = cols[[P[i], i]]
    A = dev.DMat.from_words(s, n)
    dev.apply_p(A, P, right=True)
    assert np.array_equal(dev.gather_cols(S, cols)[0].to_words(), A.to_words())


# ---- stream order, dirty scratch ----------------------------------------------------------------------------------------------------

def packed_ints(idx):
    v = np.zeros((len(idx) + 1) // 2 * 2, dtype=np.int32)
    v[:len(idx)] = idx
    return v.view(np.uint64).reshape(1, -1)


@pytest.mark.parametrize("axis", [0, 1], ids=["rows", "cols"])
def test_behind_pending_work_on_a_caller_stream(dev, axis):
    """source, destination and index array are written by copies that wait behind a sleep on the caller's stream: a step on another
    stream, or a wait on the host, would see the poison"""
    rng = np.random.default_rng(10)
    if axis == 0:
        (dn, dc), (sn, sc) = (300, 191), (129, 191)
        idx = rng.integers(-1, sn, dn)
    else:
        (dn, dc), (sn, sc) = (130, 270), (130, 200)
        idx = rng.integers(-1, sc, dc)
    s, d0 = g.random_words(sn, sc, 71), g.random_words(dn, dc, 72)
    bits = gathered_bits(g.words_to_bits(s, sc), idx, axis, len(idx))[0]
    want = g.bits_to_words(bits)
    if axis == 0:
        want = d0 ^ want   # accumulate: the destination's own content is an input too

    def issue(ls):
        (lane,) = ls
        ts, td, ti = lane.live
        S = dev.DMat.wrap(ts.data_ptr(), sn, sc, ts.shape[1], keep=ts)
        D = dev.DMat.wrap(td.data_ptr(), dn, dc, td.shape[1], keep=td)
        if axis == 0:
            dev.gather_rows(S, ti.data_ptr(), D=D, accumulate=True, stream=lane.handle)
        else:
            dev.gather_cols(S, ti.data_ptr(), D=D, stream=lane.handle)

    def check(_, reads):
        ((rs, rd, ri),) = reads
        assert np.array_equal(rd[:, :want.shape[1]], want)
        assert np.array_equal(rs[:, :s.shape[1]], s)

    from stream_util import padded
    run_pending([[padded(s), padded(d0), packed_ints(idx)]], issue, check)


def test_composed_route_on_dirty_scratch(dev, L):
    """the two scratch matrices of the composed route come from a cache in which every block holds a pattern"""
    import torch
    rows, sc, dc = 70, first_composed(dev), 200
    a = g.random_words(rows, sc, 81)
    idx = np.random.default_rng(12).integers(-1, sc, dc)
    want = g.bits_to_words(gathered_bits(g.words_to_bits(a, sc), idx, 1, dc)[0])
    for pattern in dp.PATTERNS:
        pool = dp.Pool(L, pattern)
        stream = torch.cuda.Stream().cuda_stream   # a caller stream: its arenas are new
        S = dp.dmat(a, sc, dp.pad_word(pattern))
        h0, k0 = pool.hits(), census(L)
        D, _ = dev.gather_cols(S, idx, stream=stream)
        hits, k1 = pool.hits() - h0, census(L)
        assert np.array_equal(D.to_words(stream), want)
        dp.unchanged(S, stream)
        assert_route(k0, k1, ["gf2_transpose", "gf2_gather_rows_kernel"])
        pool.no_fresh("composed column gather")
        assert hits >= 3, hits   # the index array, D and the two scratch matrices
    gc.collect()
    L.gf2_trim()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_pooled_gauss_round(dev):
    """40 systems of 20 pool rows each, gathered into a stack by device indices and eliminated in one batch"""
    batch, m, n, pool_rows = 40, 20, 24, 500
    pool = g.random_words(pool_rows, n, 91)
    pool[::7] = pool[3]   # repeated samples: some systems lose rank
    idx = np.random.default_rng(14).integers(0, pool_rows, batch * m)
    P = dev.DMat.from_words(pool, n)
    ti = ints_to_gpu(idx)
    stack, _ = dev.gather_rows(P, ti.data_ptr(), D=dev.DMat(batch * m, n))
    ranks, _ = dev.echelonize_batch(stack, m, full=True, pivots=dev.SKIP)
    got = stack.to_words()
    seen = set()
    for b in range(batch):
        red, rank, _ = g.o_echelonize(pool[idx[b * m:(b + 1) * m]], m, n, full=True)
        assert ranks[b] == rank, (b, ranks[b], rank)
        assert np.array_equal(got[b * m:(b + 1) * m], red), b
        seen.add(rank)
    assert len(seen) > 1, seen   # the round has systems of different ranks
