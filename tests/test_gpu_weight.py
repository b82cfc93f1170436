"""GPU tests of gf2_row_weights_dev, gf2_col_weights_dev, gf2_count_ones_dev and gf2_select_weights_dev (include/m4ri_hip_weight.h;
kernels: m4ri-rust_amd/csrc/weight) through device.row_weights / col_weights / count_ones / select_weights.  Expected values come from
numpy on the host (np.unpackbits through gf2util.words_to_bits, sums of the unpacked bits), independent of the library.  Outputs are raw
device arrays between two sentinels that hold a non-zero pattern before the call: the entries overwrite, the caller zeroes nothing.

Operands come in two kinds: `plain`, a buffer of its own with an even row stride on a 16-byte boundary (16-byte loads), and `view`, an
odd row stride at an odd word inside a parent full of random bits, the excess bits of the view's last word random too (8-byte loads).
Every case checks sum(row weights) == sum(column weights) == total and that the operand's whole buffer is unchanged.

Together the cases launch every kernel and every template instance of csrc/weight (tests/test_zz_kernel_census.py); the route checks
name them."""
import ctypes
import gc

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import limits_ref as lr
from census_util import assert_route, census
from stream_util import padded, run_pending

pytestmark = pytest.mark.gpu

SENT = 0x5EAD5EAD   # what an output holds before the call


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


def dirty(nrows, ld, seed):
    return g.splitmix64(seed, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld)


class Operand:
    """`words` (nrows x width(ncols)) on the device, as a buffer of its own or as a view of a dirty parent whose excess bits are dirty
    too; .host is what the whole buffer holds"""

    def __init__(self, dev, words, ncols, view, seed):
        nrows, w = words.shape
        if view:
            ld = w + 3 if (w + 3) & 1 else w + 4
            r0, c0 = 1, 2                       # word r0 * ld + c0 of the parent: odd
            self.host = dirty(nrows + 3, ld, seed)
            words = words.copy()
            if ncols % 64 and nrows:
                words[:, -1] |= dirty(nrows, 1, seed + 1)[:, 0] & ~np.uint64((1 << (ncols % 64)) - 1)
        else:
            ld = max((w + 1) & ~1, 1)
            r0, c0 = 0, 0
            self.host = dirty(max(nrows, 1), ld, seed)[:nrows]
        self.host[r0:r0 + nrows, c0:c0 + w] = words
        self.t = to_gpu(self.host) if self.host.size else None
        base = self.t.data_ptr() if self.t is not None else 0
        self.m = dev.DMat.wrap(base + 8 * (r0 * ld + c0) if base else 0, nrows, ncols, ld, keep=self.t)

    def unchanged(self):
        if self.t is not None:
            assert np.array_equal(self.t.cpu().numpy().view(np.uint64).reshape(self.host.shape), self.host), "the operand changed"


def guarded(n):
    """n device ints behind one sentinel and before another, all holding SENT; -> (tensor, address of the n ints)"""
    import torch
    t = torch.full((n + 2,), SENT, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 4


def read_guarded(t):
    h = t.cpu().numpy()
    assert h[0] == SENT and h[-1] == SENT, "a word next to the output was written"
    return h[1:-1]


def device_weights(dev, M, what, stream=None):
    import torch
    t, p = guarded(M.nrows if what == "rows" else M.ncols)
    torch.cuda.synchronize()
    assert (dev.row_weights if what == "rows" else dev.col_weights)(M, out=p, stream=stream) is None
    torch.cuda.synchronize()
    return read_guarded(t)


def content_words(kind, nrows, ncols, seed):
    if kind == "random":
        return g.random_words(nrows, ncols, seed) if nrows and ncols else np.zeros((nrows, g.width(ncols)), dtype=np.uint64)
    w = np.zeros((nrows, g.width(ncols)), dtype=np.uint64)
    if kind == "ones" and ncols:
        w[:] = ~np.uint64(0)
        if ncols % 64:
            w[:, -1] = np.uint64((1 << (ncols % 64)) - 1)
    return w


def expected(words, nrows, ncols, kind):
    if kind == "zeros":
        return np.zeros(nrows, dtype=np.int64), np.zeros(ncols, dtype=np.int64)
    if kind == "ones":
        return np.full(nrows, ncols, dtype=np.int64), np.full(ncols, nrows, dtype=np.int64)
    bits = g.words_to_bits(words, ncols) if nrows and ncols else np.zeros((nrows, ncols), dtype=np.uint8)
    return bits.sum(axis=1, dtype=np.int64), bits.sum(axis=0, dtype=np.int64)


def check_all(dev, nrows, ncols, kind, view, seed=1, what=("rows", "cols", "total")):
    """rows, columns and total of one operand against numpy, and against each other"""
    words = content_words(kind, nrows, ncols, seed)
    want_r, want_c = expected(words, nrows, ncols, kind)
    A = Operand(dev, words, ncols, view, seed + 50)
    sums = {int(want_r.sum())}
    if "rows" in what:
        got = device_weights(dev, A.m, "rows")
        bad = np.flatnonzero(got != want_r)
        assert not len(bad), "%d x %d %s: %d wrong row weights, first: row %d is %d, want %d" % (
            nrows, ncols, kind, len(bad), bad[0], got[bad[0]], want_r[bad[0]])
        sums.add(int(got.sum(dtype=np.int64)))
    if "cols" in what:
        got = device_weights(dev, A.m, "cols")
        bad = np.flatnonzero(got != want_c)
        assert not len(bad), "%d x %d %s: %d wrong column weights, first: column %d is %d, want %d" % (
            nrows, ncols, kind, len(bad), bad[0], got[bad[0]], want_c[bad[0]])
        sums.add(int(got.sum(dtype=np.int64)))
    if "total" in what:
        sums.add(dev.count_ones(A.m))
    assert len(sums) == 1, "rows, columns and total disagree: %s" % sorted(sums)
    A.unchanged()


def ran(L, k0):
    k1 = census(L)
    return sorted(k for k, v in k1.items() if v > k0.get(k, 0))


def row_threshold(dev):
    """the first ncols of the second row variant, from the plan"""
    lo, hi = 1, 1 << 24
    v0 = dev.weights_plan("rows", 100, lo)[0]
    assert dev.weights_plan("rows", 100, hi)[0] != v0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if dev.weights_plan("rows", 100, mid)[0] == v0 else (lo, mid)
    return hi


# ---- rows, and the total on the same operands ---------------------------------------------------------------------------------------

ROW_COUNTS = (1, 5, 64, 65, 300)
ROW_WIDTHS = (1, 63, 64, 65, "T-1", "T", "T+1", 4097, 70001)


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("ncols", ROW_WIDTHS, ids=str)
def test_rows(dev, L, ncols, view):
    T = row_threshold(dev)
    if isinstance(ncols, str):
        ncols = T + {"T-1": -1, "T": 0, "T+1": 1}[ncols]
    k0 = census(L)
    for nrows in ROW_COUNTS:
        for kind in ("random", "zeros", "ones"):
            check_all(dev, nrows, ncols, kind, view, seed=3 * nrows, what=("rows", "total"))
    kernels = ran(L, k0)
    narrow = [k for k in kernels if "gf2_weight_rows_narrow_kernel" in k]
    wide = [k for k in kernels if "gf2_weight_rows_wide_kernel" in k]
    assert (bool(narrow), bool(wide)) == ((True, False) if ncols < T else (False, True)), kernels
    assert dev.weights_plan("rows", 5, ncols)[0] == (0 if ncols < T else 1)
    assert [k for k in kernels if "gf2_weight_total_kernel" in k], kernels


def test_rows_and_total_reach_every_instance(dev, L):
    """8 and 64 lanes per row, 1, 8 and 64 lanes in the total: the widths above, named by the plan"""
    T = row_threshold(dev)
    seen = set()
    for ncols in (65, T, 4097):
        p, q = dev.weights_plan("rows", 300, ncols), dev.weights_plan("total", 300, ncols)
        k0 = census(L)
        check_all(dev, 300, ncols, "random", False, seed=9, what=("rows", "total"))
        seen |= set(ran(L, k0))
        assert 256 % p[2] == 0 and q[2] == p[2]   # rows per workgroup: 256 / lanes per row
    for inst in ("rows_wide_kernelILi8E", "rows_wide_kernelILi64E", "total_kernelILi1E", "total_kernelILi8E", "total_kernelILi64E"):
        assert [k for k in seen if inst in k], (inst, sorted(seen))


# ---- columns --------------------------------------------------------------------------------------------------------------------------

COL_SHAPES = [(1, 1), (1, 64), (63, 65), (64, 64), (65, 129), (1000, 191), (257, 4097), (3, 70001), (65536, 256)]


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("shape", COL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_cols(dev, L, shape, view):
    nrows, ncols = shape
    k0 = census(L)
    for kind in ("random", "ones"):
        check_all(dev, nrows, ncols, kind, view, seed=5)
    kernels = ran(L, k0)
    assert [k for k in kernels if "gf2_weight_cols_kernelILb%dE" % (0 if view or ncols <= 64 else 1) in k], kernels
    variant, _, _, _, scratch = dev.weights_plan("cols", nrows, ncols)
    assert bool([k for k in kernels if "gf2_weight_fold_kernel" in k]) == (variant == 1) == (scratch > 0), kernels


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("ncols", [65, 256])
def test_cols_around_the_pass_and_the_flush_period(dev, L, ncols, view):
    """R rows per pass of a workgroup, F rows of a lane between two flushes of its counter planes (both from the plan): row counts on
    both sides of R, of F, of F * R -- where the first lane takes its row F + 1 and has to have emptied its planes -- and of the row
    count at which the rows are cut into two bands, and more.  With all-ones content every column weight is the row count: a counter
    that wraps, or a flush that is lost, shows there."""
    _, threads, R, F, _ = dev.weights_plan("cols", 1000, ncols)
    assert R > 0 and F > 0 and threads % R == 0
    two_bands = next(n for n in range(R, 1 << 22, R) if dev.weights_plan("cols", n + 1, ncols)[0] == 1)
    assert two_bands > F * R   # a lane of a single band passes the flush period before the rows are cut
    counts = [R - 1, R, R + 1, F - 1, F, F + 1, 2 * F + 1, F * R - 1, F * R, F * R + 1, F * R + 8 * R + 1, two_bands, two_bands + 1,
              2 * F * R + 1, 8 * F * R + 3]
    variants = set()
    for nrows in counts:
        variants.add(dev.weights_plan("cols", nrows, ncols)[0])
        for kind in ("ones", "random"):
            check_all(dev, nrows, ncols, kind, view, seed=7, what=("cols", "total"))
    assert variants == {0, 1}


def test_cols_of_a_matrix_without_rows_and_rows_of_one_without_columns(dev):
    import torch
    for nrows, ncols, what in ((0, 200, "cols"), (200, 0, "rows")):
        M = dev.DMat.wrap(0, nrows, ncols, 4)
        got = device_weights(dev, M, what)
        assert len(got) == 200 and not got.any()      # zeros are written: the sentinel pattern is gone
        assert dev.count_ones(M) == 0
    assert len(dev.row_weights(dev.DMat.wrap(0, 0, 200, 4))) == 0 and len(dev.col_weights(dev.DMat.wrap(0, 200, 0, 4))) == 0
    # the wrappers that allocate their own output, and the DMat methods
    a = g.random_words(70, 130, 3)
    A = dev.DMat.from_words(a, 130)
    want_r, want_c = expected(a, 70, 130, "random")
    assert np.array_equal(A.row_weights(), want_r) and np.array_equal(A.col_weights(), want_c) and A.count_ones() == want_r.sum()
    v = dev.DMat.from_words(a[:1], 130)
    assert v.count_ones() == want_r[0]                # a vector: the reference's count_ones
    torch.cuda.synchronize()


# ---- the total past 2^32 --------------------------------------------------------------------------------------------------------------

def test_total_past_2_to_32(dev, L):
    """all ones, 70 001 x 70 001 = 4.9e9 bits, every word of the buffer all ones (the excess bits of the last word and the pad word
    too): the total is nrows * ncols exactly, every row and column weight 70 001"""
    import torch
    n = 70001
    ld = (g.width(n) + 1) & ~1
    t = torch.full((n, ld), -1, dtype=torch.int64, device="cuda")
    A = dev.DMat.from_torch(t, n)
    assert n * n > 1 << 32
    assert dev.count_ones(A) == n * n
    rows, cols = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.row_weights(A, out=rows.data_ptr())
    dev.col_weights(A, out=cols.data_ptr())
    torch.cuda.synchronize()
    assert bool((rows == n).all()) and bool((cols == n).all())
    del A, t
    gc.collect()


# ---- select ---------------------------------------------------------------------------------------------------------------------------

def select_case(dev, w, lo, hi, cap):
    """one call with raw device arrays; cap None: a count-only call with idx NULL"""
    import torch
    n = len(w)
    tw = ints_to_gpu(w)
    ti, pi = guarded(cap or 0)
    tc, pc = guarded(1)
    torch.cuda.synchronize()
    out = dev.select_weights(tw.data_ptr(), n, lo, hi, idx=dev.SKIP if cap is None else pi, cap=0 if cap is None else cap, count=pc)
    assert out == (None, None)
    torch.cuda.synchronize()
    want = np.flatnonzero((w >= lo) & (w <= hi))
    count = int(read_guarded(tc)[0])
    assert count == len(want), (n, lo, hi, cap, count, len(want))
    got = read_guarded(ti)
    k = min(count, cap or 0)
    assert np.array_equal(got[:k], want[:k]), (n, lo, hi, cap)
    assert np.all(np.diff(got[:k]) > 0)
    assert np.all(got[k:] == SENT), "entries behind min(count, cap) were written"
    assert np.array_equal(tw.cpu().numpy(), w), "the weights changed"
    return got.copy(), count


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 100003])
def test_select(dev, L, n):
    rng = np.random.default_rng(n)
    w = rng.integers(10, 1000, n).astype(np.int32)
    w[0], w[n - 1] = 5, (2000 if n > 1 else 5)
    windows = {"nothing": (1001, 1999), "empty window": (600, 400), "everything": (0, 2000), "index 0": (5, 5), "index n-1": (2000, 2000) if n > 1 else (5, 5),
               "half": (10, 505), "negative": (-(1 << 31), -1), "all ints": (-(1 << 31), (1 << 31) - 1)}
    k0 = census(L)
    for name, (lo, hi) in windows.items():
        matches = int(np.count_nonzero((w >= lo) & (w <= hi)))
        for cap in sorted({None, 1, max(matches - 1, 0), matches, matches + 5}, key=lambda c: -1 if c is None else c):
            first = select_case(dev, w, lo, hi, cap)
            again = select_case(dev, w, lo, hi, cap)
            assert np.array_equal(first[0], again[0]) and first[1] == again[1], name
    assert_route(k0, census(L), ["gf2_weight_select_count_kernel", "gf2_weight_select_scan_kernel", "gf2_weight_select_scatter_kernel"])


def test_select_wrapper_and_empty_input(dev):
    import torch
    w = np.array([7, 1, 7, 9, 0, 7], dtype=np.int32)
    idx, count = dev.select_weights(w, len(w), 7, 7)
    assert count == 3 and list(idx) == [0, 2, 5]
    idx, count = dev.select_weights(list(w), len(w), 0, 1, cap=1)
    assert count == 2 and list(idx) == [1]
    assert dev.select_weights(w, len(w), 0, 9, idx=dev.SKIP) == (None, 6)
    # n == 0 with room in idx: *count = 0 is written, idx is not touched
    ti, pi = guarded(4)
    tc, pc = guarded(1)
    torch.cuda.synchronize()
    dev.select_weights(0, 0, 0, 9, idx=pi, cap=4, count=pc)
    torch.cuda.synchronize()
    assert read_guarded(tc)[0] == 0 and np.all(read_guarded(ti) == SENT)


# ---- limits ---------------------------------------------------------------------------------------------------------------------------

def test_past_the_row_limit(dev, L):
    """4 194 369 x 65 (more than 2^22 rows), built on the device from a period of 4099 random rows: the expectation comes from one
    period"""
    import torch
    R, n, P = lr.R, 65, 4099
    period = g.random_words(P, n, 77)
    tp = to_gpu(padded(period))
    t = tp[torch.arange(R, device="cuda") % P].contiguous()
    A = dev.DMat.from_torch(t, n)
    bits = g.words_to_bits(period, n)
    pr = bits.sum(axis=1, dtype=np.int64)
    want_c = (R // P) * bits.sum(axis=0, dtype=np.int64) + bits[:R % P].sum(axis=0, dtype=np.int64)
    rows = torch.full((R,), SENT, dtype=torch.int32, device="cuda")
    cols, pc = guarded(n)
    torch.cuda.synchronize()
    dev.row_weights(A, out=rows.data_ptr())
    dev.col_weights(A, out=pc)
    total = dev.count_ones(A)
    got_r = rows.cpu().numpy()
    assert np.array_equal(got_r, pr[np.arange(R) % P])
    assert np.array_equal(read_guarded(cols), want_c)
    assert total == int(want_c.sum()) == int(got_r.sum(dtype=np.int64))
    # the flush period is passed at this size, in more than one band
    variant, _, rows_per_pass, F, scratch = dev.weights_plan("cols", R, n)
    assert variant == 1 and R > scratch // (4 * n) * F * rows_per_pass
    del A, t
    gc.collect()


def test_an_operand_past_4gib(dev, L):
    """8 400 000 x 4096 (4.3 GB) from gf2_dmat_fill_random: the three sums agree, and rows from the first, the middle and the last 1 %
    (both sides of byte offset 2^32 among them) have exactly the weight of a downloaded window"""
    import torch
    m, n, seed = 8_400_000, 4096, 0x71E
    gc.collect()
    L.gf2_trim()
    A = dev.DMat.random(m, n, seed)
    assert m * A.ld * 8 > lr.LIMIT_BYTES
    rows = torch.full((m,), SENT, dtype=torch.int32, device="cuda")
    cols, pc = guarded(n)
    torch.cuda.synchronize()
    dev.row_weights(A, out=rows.data_ptr())
    dev.col_weights(A, out=pc)
    total = dev.count_ones(A)
    got_c = read_guarded(cols)
    assert total == int(rows.sum(dtype=torch.int64).item()) == int(got_c.sum(dtype=np.int64))
    assert abs(total - m * n // 2) < 1 << 24 and got_c.min() > m // 2 - (1 << 16) and got_c.max() < m // 2 + (1 << 16)
    rng = np.random.default_rng(3)
    picks = np.unique(np.concatenate([rng.integers(0, m // 100, 8), m // 2 + rng.integers(0, m // 100, 8), m - 1 - rng.integers(0, m // 100, 8),
                                      [0, m - 1], lr.straddle(A.ld, m)]))
    window = lr.fetch_rows(dev, A, picks)
    want = g.words_to_bits(window, n).sum(axis=1, dtype=np.int64)
    assert np.array_equal(window, lr.seeded_words(seed, n, picks))
    assert np.array_equal(rows[torch.from_numpy(picks).cuda()].cpu().numpy(), want)
    del A, rows
    gc.collect()
    L.gf2_trim()


# ---- stream order, dirty scratch ----------------------------------------------------------------------------------------------------

def packed_ints(count, fill=0):
    return np.full((1, (count + 1) // 2), np.uint64(fill), dtype=np.uint64)


def test_behind_pending_work_on_a_caller_stream(dev):
    """the operand is written by a copy that waits behind a sleep on the caller's stream, the outputs hold poison until the calls run
    there: rows, columns, total; then the selection reads the row weights and the row gather reads the selected indices, all enqueued
    before anything synchronises.  A step on another stream, or a wait on the host, would see the poison."""
    m, n = 3000, 517     # columns in several bands (scratch and the fold launch), rows on the 8-lane kernel
    a = g.random_words(m, n, 61)
    bits = g.words_to_bits(a, n)
    want_r, want_c = bits.sum(axis=1, dtype=np.int64), bits.sum(axis=0, dtype=np.int64)
    lo, hi = 0, int(np.sort(want_r)[40])
    hits = np.flatnonzero((want_r >= lo) & (want_r <= hi))
    cap = len(hits) + 3
    assert dev.weights_plan("cols", m, n)[0] == 1

    def issue(ls):
        (lane,) = ls
        ta, tr, tc, tt, ti, tn, tg = lane.live
        A = dev.DMat.wrap(ta.data_ptr(), m, n, ta.shape[1], keep=ta)
        G = dev.DMat.wrap(tg.data_ptr(), cap, n, tg.shape[1], keep=tg)
        s = lane.handle
        dev.row_weights(A, out=tr.data_ptr(), stream=s)
        dev.col_weights(A, out=tc.data_ptr(), stream=s)
        dev._lib.check(dev._lib.lib().gf2_count_ones_dev(A._on(s), tt.data_ptr(), s), "gf2_count_ones_dev")
        dev.select_weights(tr.data_ptr(), m, lo, hi, idx=ti.data_ptr(), cap=cap, count=tn.data_ptr(), stream=s)
        dev.gather_rows(A, ti.data_ptr(), D=G, stream=s)

    def check(_, reads):
        ((ra, rr, rc, rt, ri, rn, rg),) = reads
        assert np.array_equal(rr.view(np.int32).reshape(-1)[:m], want_r)
        assert np.array_equal(rc.view(np.int32).reshape(-1)[:n], want_c)
        assert int(rt.reshape(-1)[0]) == int(want_r.sum())
        assert int(rn.view(np.int32).reshape(-1)[0]) == len(hits)
        assert np.array_equal(ri.view(np.int32).reshape(-1)[:len(hits)], hits)
        assert np.array_equal(rg[:len(hits), :a.shape[1]], a[hits])
        assert not rg[len(hits):, :a.shape[1]].any()     # the -1 the test put behind the hits: zero rows
        assert np.array_equal(ra[:, :a.shape[1]], a)

    idx0 = np.full(cap + (cap & 1), -1, dtype=np.int32).view(np.uint64).reshape(1, -1)   # behind min(count, cap): untouched, so -1
    run_pending([[padded(a), packed_ints(m), packed_ints(n), packed_ints(2), idx0, packed_ints(2), np.zeros((cap, padded(a).shape[1]), dtype=np.uint64)]],
                issue, check)


def test_on_dirty_scratch(dev, L):
    """the per-band column sums and the block counts of the selection come from a cache in which every block holds a pattern, and no
    block comes fresh from the driver during the calls; the other plans take no scratch at all"""
    import torch
    m, n = 9000, 700
    a = g.random_words(m, n, 81)
    bits = g.words_to_bits(a, n)
    want_r, want_c = bits.sum(axis=1, dtype=np.int64), bits.sum(axis=0, dtype=np.int64)
    variant, _, _, _, scratch = dev.weights_plan("cols", m, n)
    assert variant == 1 and scratch > 4 * n
    for what in ("rows", "total"):
        for shape in ((m, n), (1 << 20, 256), (65536, 65536), (3, 70001)):
            assert dev.weights_plan(what, *shape)[4] == 0
    lo, hi = int(np.median(want_r)), int(want_r.max())
    hits = np.flatnonzero((want_r >= lo) & (want_r <= hi))
    for pattern in dp.PATTERNS:
        pool = dp.Pool(L, pattern)
        stream = torch.cuda.Stream().cuda_stream   # a caller stream: its arenas are new
        A = dp.dmat(a, n, dp.pad_word(pattern))
        h0, k0 = pool.hits(), census(L)
        got_c = dev.col_weights(A, stream=stream)
        got_r = dev.row_weights(A, stream=stream)
        idx, count = dev.select_weights(got_r, m, lo, hi, stream=stream)
        hits_taken = pool.hits() - h0
        assert np.array_equal(got_c, want_c) and np.array_equal(got_r, want_r)
        assert count == len(hits) and np.array_equal(idx, hits)
        assert dev.count_ones(A, stream=stream) == int(want_r.sum())
        dp.unchanged(A, stream)
        assert_route(k0, census(L), ["gf2_weight_cols_kernel", "gf2_weight_fold_kernel", "gf2_weight_select_scan_kernel"])
        pool.no_fresh("weights on dirty scratch")
        assert hits_taken >= 2, hits_taken   # the partial sums and the block counts, besides the wrappers' own arrays
    gc.collect()
    L.gf2_trim()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_lpn_verdict_on_the_device(dev):
    """4096 samples of 64 bits with labels of noise rate 1/8 and 64 candidate secrets, one of them the true one: E = [samples | labels] *
    [S ; 1] is one product, the weight of column b of E the number of samples candidate b gets wrong; the selection below N / 4 yields
    exactly the true candidate"""
    import torch
    N, k, V, true_at = 4096, 64, 64, 37
    rng = np.random.default_rng(2026)
    samples = rng.integers(0, 2, (N, k), dtype=np.uint8)
    secret = rng.integers(0, 2, k, dtype=np.uint8)
    noise = (rng.random(N) < 1 / 8).astype(np.uint8)
    labels = (samples @ secret + noise) % 2
    cand = rng.integers(0, 2, (k, V), dtype=np.uint8)
    cand[:, true_at] = secret
    pool_bits = np.concatenate([samples, labels[:, None].astype(np.uint8)], axis=1)          # N x (k + 1)
    s1_bits = np.concatenate([cand, np.ones((1, V), dtype=np.uint8)], axis=0)                 # (k + 1) x V
    want = ((pool_bits.astype(np.int64) @ s1_bits.astype(np.int64)) % 2).sum(axis=0)
    assert want[true_at] == noise.sum() < N // 4 and np.all(np.delete(want, true_at) >= N // 4)
    pool = dev.DMat.from_words(g.bits_to_words(pool_bits), k + 1)
    S1 = dev.DMat.from_words(g.bits_to_words(s1_bits), V)
    weights, pw = guarded(V)
    found, pf = guarded(V)
    count, pc = guarded(1)
    torch.cuda.synchronize()
    E = dev.mul(pool, S1)
    dev.col_weights(E, out=pw)
    dev.select_weights(pw, V, 0, N // 4 - 1, idx=pf, cap=V, count=pc)
    torch.cuda.synchronize()
    assert np.array_equal(read_guarded(weights), want)
    assert read_guarded(count)[0] == 1 and read_guarded(found)[0] == true_at and np.all(read_guarded(found)[1:] == SENT)
