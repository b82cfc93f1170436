"""GPU tests of include/m4ri_hip_find.h: gf2_find_rows_dev bit for bit against the numpy yardstick of tests/find_ref.py (itself checked
against a double loop by tests/test_find_reference.py) and, for A is B, against gf2_unique_rows_dev on the device: `idx`, `mult` and
`count`, all of them exactly.

The harness is that of tests/test_gpu_unique.py: A and B are windows of dirty parents (View of tests/test_gpu_lf1.py: the excess bits
of the last word are dirty too) and the parents are compared afterwards; the int outputs lie between sentinels and hold a pattern
before the call; which kernels ran, and how many launches a call took, is read from the launch census and compared with
gf2_find_rows_plan.

The pools (pools()): B is a pool of tests/test_gpu_unique.py -- rows drawn from a dictionary of about NB / 3 values of the range, so
classes have several members scattered through the pool, junk outside the range --; every second row of A holds the range of a row of
B and every other one fresh bits; for every column of the range one of the fresh rows is a row of B with that column alone flipped,
which must not match; and a row of A equals a row of B on the range and differs from it in the columns c0 - 1 and c1, which must."""
import gc

import numpy as np
import pytest

import dev_views as dv
import dirty_pool as dp
import find_ref as fr
import gf2util as g
import limits_ref as lr
import unique_ref as ur
from census_util import assert_route, census
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded
from test_gpu_unique import RANGES, pool, pool_bits, with_values

pytestmark = pytest.mark.gpu

BIG = 3 * 4096 + 5
FILL = "gf2_find_fill_kernel"
BUILD = {0: "gf2_find_build_kernelILb0EE", 1: "gf2_find_build_kernelILb1EE"}     # a lane per row, a wave per row
LOOKUP = {0: "gf2_find_lookup_kernelILb0EE", 1: "gf2_find_lookup_kernelILb1EE"}
LAYOUTS4 = [EE, EO, OE, OO]


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


# ---- pools -----------------------------------------------------------------------------------------------------------------------

def pools(na, nb, ncols, c0, c1, seed):
    """-> (bits of A, bits of B, src): (n, ncols) uint8 as the module docstring says; src[i]: the row of B that row i of A was made of"""
    rng = np.random.default_rng(seed)
    b = pool_bits(nb, ncols, c0, c1, seed + 1)
    a = rng.integers(0, 2, (na, ncols), dtype=np.uint8)
    src = rng.integers(0, max(nb, 1), na)
    w = c1 - c0
    if nb and na and w:
        hit = np.arange(na) % 2 == 0
        a[hit, c0:c1] = b[src[hit], c0:c1]
        odd = np.arange(1, na, 2)
        for t, i in enumerate(odd[:min(w, len(odd) // 2)]):                     # column c0 + t alone differs; half the odd rows stay fresh
            a[i, c0:c1] = b[src[i], c0:c1]
            a[i, c0 + t] ^= 1
        i = (na - 1) & ~1                                                       # a hit that differs right outside the range
        if c0 > 0:
            a[i, c0 - 1] = b[src[i], c0 - 1] ^ 1
        if c1 < ncols:
            a[i, c1] = b[src[i], c1] ^ 1
    return a, b, src


def to_words(bits, ncols):
    return g.bits_to_words(bits) if ncols else np.zeros((len(bits), 0), dtype=np.uint64)


def launches(before, after, family=""):
    return sum(v - before.get(k, 0) for k, v in after.items() if family in k)


def run(dev, L, aw, bw, ncols, c0, c1, la=EE, lb=OO, mult=True, count=True, stream=None, want=None, ncols_b=None):
    """gf2_find_rows_dev on two dirty windows against the yardstick -> the yardstick's result"""
    import torch
    na, nb = len(aw), len(bw)
    ncols_b = ncols if ncols_b is None else ncols_b
    if want is None:
        want = fr.find_rows(aw, bw, c0, c1)
    A, B = View(dev, na, ncols, la, 5 * na + c0, aw), View(dev, nb, ncols_b, lb, 7 * nb + c1, bw)
    (ti, pi), (tm, pm), (tc, pc) = guarded(na), guarded(na), guarded(1)
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.find_rows(A.m, B.m, c0, c1, idx=pi, mult=pm if mult else dev.SKIP, count=pc if count else dev.SKIP, stream=stream)
    assert out == (None, None, None)
    torch.cuda.synchronize()
    k1 = census(L)
    what = (na, nb, ncols, ncols_b, c0, c1, la, lb, mult, count)
    idx, mults, counts = (read_guarded(t) for t in (ti, tm, tc))
    assert np.array_equal(idx, want.idx), (what, np.flatnonzero(idx != want.idx)[:8])
    assert np.array_equal(mults, want.mult if mult else np.full(na, SENT)), (what, np.flatnonzero(mults != want.mult)[:8])
    assert int(counts[0]) == (want.count if count else SENT), (what, counts[0], want.count)
    A.unchanged()
    B.unchanged()
    plan = dev.find_rows_plan(na, nb, min(ncols, ncols_b), c0, c1)
    assert launches(k0, k1) == plan[4] == (3 if na and nb else 0), (what, launches(k0, k1), plan)
    if na and nb:
        assert_route(k0, k1, [FILL, BUILD[plan[7]], LOOKUP[plan[7]]])
        assert launches(k0, k1, "gf2_find_") == 3 and launches(k0, k1, BUILD[1 - plan[7]]) == 0, what
    return want


# ---- row counts --------------------------------------------------------------------------------------------------------------------

def test_the_sizes_are_the_plans(dev):
    assert dev.find_rows_plan(1000, 1000, 200, 57, 200)[5:] == (256, 256, 0, 4) and dev.find_rows_plan(1000, 1000, 1000, 3, 997)[5:] == (64, 64, 1, 16)


SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, BIG]
PAIRS = [(n, n) for n in SIZES] + [(0, 5), (5, 0), (1, BIG), (BIG, 1), (2, 63), (65, 1025), (4097, 64), (1023, BIG), (BIG, 1024)]


@pytest.mark.parametrize("sizes", PAIRS, ids=lambda s: "%dx%d" % s)
def test_row_counts(dev, L, sizes):
    na, nb = sizes
    ncols, c0, c1 = 200, 57, 200
    a, b, _ = pools(na, nb, ncols, c0, c1, 100 + na + 3 * nb)
    want = run(dev, L, to_words(a, ncols), to_words(b, ncols), ncols, c0, c1, la=LAYOUTS4[na % 4], lb=LAYOUTS4[nb % 4])
    if na >= 64 and nb >= 64:
        assert 0 < want.count < na and want.mult.max() > 1                     # hits and misses, and classes of several members
    if nb == 0:
        assert want.count == 0 and (want.idx == -1).all() and not want.mult.any()


# ---- ranges ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RANGES, ids=lambda c: "%d-c%d-%d" % c)
def test_ranges(dev, L, case):
    """one bit, one word, the empty range, ranges that cross words, four and five words (a lane per row) and sixteen (a wave per row);
    5000 rows a side: twenty workgroups of the lane form, and room for a planted row per column of the widest range"""
    ncols, c0, c1 = case
    n = 5000
    a, b, src = pools(n, n, ncols, c0, c1, 7 * ncols + c0)
    k = RANGES.index(case)
    want = run(dev, L, to_words(a, ncols), to_words(b, ncols), ncols, c0, c1, la=LAYOUTS4[k % 4], lb=LAYOUTS4[(k + 1) % 4])
    assert dev.find_rows_plan(n, n, ncols, c0, c1)[7] == (1 if case == (1000, 3, 997) else 0)
    if c0 == c1:
        assert want.count == n and not want.idx.any() and (want.mult == n).all()
        return
    # what the pools promise, read off the yardstick: a hit agrees with its row of B on the range ...
    found = want.idx >= 0
    assert np.array_equal(b[want.idx[found], c0:c1], a[found, c0:c1]) and found[::2].all()
    planted = np.arange(1, n, 2)[:min(c1 - c0, n // 4)]
    assert (want.idx[planted] != src[planted]).all()                           # ... one flipped column is no match ...
    if c1 - c0 >= 64:
        assert 0 < want.count < n and not found[1::2][-n // 8:].any()          # the fresh rows are misses
    i = (n - 1) & ~1                                                            # ... and the columns next to the range do not count
    assert found[i] and np.array_equal(b[want.idx[i], c0:c1], b[src[i], c0:c1])
    if c0 > 0 and c1 < ncols:
        assert a[i, c0 - 1] != b[src[i], c0 - 1] and a[i, c1] != b[src[i], c1]


# ---- A is B ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(200, 57, 200), (64, 0, 64), (1000, 3, 997)], ids=lambda c: "%d-c%d-%d" % c)
def test_a_is_b_gives_the_rep_of_unique_rows(dev, case):
    ncols, c0, c1 = case
    for n in (1, 4097, BIG):
        words = pool(n, ncols, c0, c1, n + c1)
        want = fr.find_rows(words, words, c0, c1)
        P = dev.DMat.from_words(words, ncols)
        idx, mult, count = dev.find_rows(P, P, c0, c1)
        rep = dev.unique_rows(P, c0, c1, cap=n)[2]                               # on the device, in the same test
        got = idx.read(None)
        assert got.dtype == np.int32 and np.array_equal(got, rep.read(None)) and np.array_equal(got, ur.unique_rows(words, c0, c1)[2])
        assert np.array_equal(got, want.idx) and int(count.read(None)[0]) == n
        sizes = np.bincount(got, minlength=n)                                    # the members of every class, at its lowest row
        assert np.array_equal(mult.read(None), sizes[got]) and np.array_equal(sizes[got], want.mult)
        if n > 1:
            assert sizes.max() > 1


def test_a_and_b_are_two_views_of_one_parent(dev):
    n, ncols, c0, c1 = 6000, 200, 57, 200
    words = pool(n, ncols, c0, c1, 12)
    P = View(dev, n, ncols, OE, 13, words)
    ld = P.m.ld
    A = dev.DMat.wrap(P.m.s.data + 8 * ld * 100, n - 100, ncols, ld, keep=P.t)     # rows 100 .. n
    B = dev.DMat.wrap(P.m.s.data, n - 50, ncols - 7, ld, keep=P.t)                 # rows 0 .. n - 50, a narrower view
    want = fr.find_rows(words[100:], words[:n - 50], c0, c1 - 7)
    idx, mult, count = dev.find_rows(A, B, c0, c1 - 7)
    assert np.array_equal(idx.read(None), want.idx) and np.array_equal(mult.read(None), want.mult)
    assert int(count.read(None)[0]) == want.count and 0 < want.count < n - 100
    P.unchanged()


# ---- class shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["all-equal", "all-distinct", "giant-then-distinct", "disjoint", "permuted-multiset"])
def test_class_shapes(dev, L, shape):
    n, ncols, c0, c1 = BIG, 200, 57, 200
    rng = np.random.default_rng(len(shape))
    if shape == "all-equal":                                                     # BIG rows in one slot: the worst contention
        ids_b, ids_a = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    elif shape == "all-distinct":
        ids_b, ids_a = rng.permutation(n), rng.integers(0, 2 * n, n)
    elif shape == "giant-then-distinct":
        ids_b, ids_a = np.maximum(np.arange(n) - 9000, 0)[rng.permutation(n)], rng.integers(0, n - 9000 + 500, n)
    elif shape == "disjoint":
        ids_b, ids_a = rng.permutation(n), n + rng.integers(0, n, n)
    else:
        ids_b = rng.integers(0, n // 3, n)
        ids_a = ids_b[rng.permutation(n)]
    words = with_values(2 * n, ncols, c0, c1, 31 + len(shape), np.concatenate([ids_b, ids_a]))
    want = run(dev, L, words[n:], words[:n], ncols, c0, c1, la=OO, lb=EO)
    first = {}
    for j, v in enumerate(ids_b.tolist()):
        first.setdefault(v, j)
    assert want.idx.tolist() == [first.get(v, -1) for v in ids_a.tolist()]       # the ids say the same as the yardstick
    if shape == "all-equal":
        assert not want.idx.any() and (want.mult == n).all() and want.count == n
    elif shape == "all-distinct":
        assert 0 < want.count < n and set(want.mult.tolist()) == {0, 1}
    elif shape == "giant-then-distinct":
        assert want.mult.max() == 9001 and (want.idx[want.mult == 9001] == np.flatnonzero(ids_b == 0)[0]).all() and 0 < want.count < n
    elif shape == "disjoint":
        assert want.count == 0 and (want.idx == -1).all() and not want.mult.any()
    else:
        assert want.count == n and want.mult.min() >= 1 and want.mult.max() > 1


# ---- mult and count NULL -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(130, 1, 129), (1000, 3, 997)], ids=lambda c: "%d-c%d-%d" % c)
def test_mult_and_count_may_be_null(dev, L, case):
    """every combination, on both forms; a skipped output keeps its pattern and the launches stay the plan's (run() holds both)"""
    ncols, c0, c1 = case
    a, b, _ = pools(3000, 2500, ncols, c0, c1, 55)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    want = fr.find_rows(aw, bw, c0, c1)
    assert 0 < want.count < 3000 and want.mult.max() > 1
    for mult, count in ((True, True), (False, False), (True, False), (False, True)):
        run(dev, L, aw, bw, ncols, c0, c1, la=EO, lb=OE, mult=mult, count=count, want=want)


# ---- different widths and strides --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout_a", dv.LAYOUTS)
def test_different_widths_and_strides(dev, layout_a):
    """tests/dev_views.py: at least one dirty row above and two below each window, dirty words left and right of it; 8-byte-aligned
    rows, an odd ld, a base on an odd word; WIDE: a column range of a wider matrix.  A has 400 columns, B 260: other row widths and
    strides.  Nothing of the parents is written"""
    na, nb, ca, cb, c0, c1 = 1500, 1300, 400, 260, 61, 255
    a, b, _ = pools(na, nb, ca, c0, c1, 40 + dv.LAYOUTS.index(layout_a))
    A = dv.View(dev, na, ca, layout_a, 41, to_words(a, ca))
    bw = to_words(b[:, :cb], cb)
    want = fr.find_rows(A.window(), bw, c0, c1)
    assert 0 < want.count < na and want.mult.max() > 1
    for layout_b in dv.LAYOUTS:
        B = dv.View(dev, nb, cb, layout_b, 43, bw)
        assert A.ld != B.ld
        idx, mult, count = dev.find_rows(A.m, B.m, c0, c1)
        assert np.array_equal(idx.read(None), want.idx) and np.array_equal(mult.read(None), want.mult), (layout_a, layout_b)
        assert int(count.read(None)[0]) == want.count
        B.unchanged("B")
    A.unchanged("A")
    # c1 = None: to the last column of the narrower of the two
    idx, _, _ = dev.find_rows(A.m, B.m, 200, mult=dev.SKIP, count=dev.SKIP)
    assert np.array_equal(idx.read(None), fr.find_rows(A.window(), bw, 200, cb).idx)


# ---- dirty scratch, streams --------------------------------------------------------------------------------------------------------

def test_on_dirty_scratch(dev, L):
    """the table comes from a cache in which every block holds a pattern, and no block comes fresh from the driver: entries and
    counts that the call did not initialise would be read"""
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for n, ncols, c0, c1 in ((BIG, 200, 57, 200), (9000, 1000, 3, 997), (5000, 64, 0, 64)):
            a, b, _ = pools(n, n - 77, ncols, c0, c1, n)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run(dev, L, to_words(a, ncols), to_words(b, ncols), ncols, c0, c1, stream=stream, la=OE, lb=EE)
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the row lookup on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """A and B are gathered from a dictionary that gf2_dmat_fill_random writes on the caller's stream, behind a sleep; the same call
    is enqueued twice behind it, into two sets of arrays, before anything synchronises.  Both must hold what the yardstick makes of
    the seeded dictionary."""
    import torch
    n, ncols, seed, c0, c1 = 9001, 200, 0x51DE, 10, 190
    known = n // 3
    dictionary = lr.seeded_words(seed, ncols, np.arange(2 * known))
    rng = np.random.default_rng(5)
    ib, ia = rng.integers(0, known, n).astype(np.int32), rng.integers(0, 2 * known, n).astype(np.int32)
    want = fr.find_rows(dictionary[ia], dictionary[ib], c0, c1)
    assert n // 4 < want.count < 3 * n // 4 and want.mult.max() > 1
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    td = torch.full((2 * known, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ta = torch.full((n, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    tb = torch.full((n, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    tia, tib = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    S, A, B = dev.DMat.from_torch(td, ncols), dev.DMat.from_torch(ta, ncols), dev.DMat.from_torch(tb, ncols)
    outs = [[guarded(n), guarded(n), guarded(1)] for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    S.fill_random(seed, s)
    dev.gather_rows(S, tia.data_ptr(), D=A, stream=s)
    dev.gather_rows(S, tib.data_ptr(), D=B, stream=s)
    for (ti, pi), (tm, pm), (tc, pc) in outs:
        dev.find_rows(A, B, c0, c1, idx=pi, mult=pm, count=pc, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for (ti, pi), (tm, pm), (tc, pc) in outs:
        assert np.array_equal(read_guarded(ti), want.idx) and np.array_equal(read_guarded(tm), want.mult)
        assert int(read_guarded(tc)[0]) == want.count


# ---- past 4 GiB ----------------------------------------------------------------------------------------------------------------------

def test_b_is_a_view_of_a_parent_past_4gib(dev, L):
    """B: 600 rows of 200 columns, 2^20 words apart: the rows from 512 on start behind byte offset 2^32 of the parent.  Only the
    view's words are written (gf2_copy_block_dev from a compact upload).  A is compact and finds rows on both sides"""
    import torch
    n, ncols, ld, c0, c1 = 600, 200, 1 << 20, 57, 200
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        reason = "the view past 4 GiB needs 8 GiB of free device memory, %.1f GiB are free" % (free / (1 << 30))
        print(reason)
        pytest.skip(reason)
    t = torch.empty((n, ld), dtype=torch.int64, device="cuda")
    assert n * ld * 8 > lr.LIMIT_BYTES
    rng = np.random.default_rng(90)                                # B all distinct, so a hit's idx is the row it was made of
    a, b, src = rng.integers(0, 2, (400, ncols), dtype=np.uint8), rng.integers(0, 2, (n, ncols), dtype=np.uint8), rng.integers(0, n, 400)
    a[::2, c0:c1] = b[src[::2], c0:c1]
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    bw[599] = bw[3]                                                # classes with a member on either side of the boundary
    bw[7] = bw[550]
    aw[0], aw[2] = bw[599], bw[550]
    want = fr.find_rows(aw, bw, c0, c1)
    assert want.idx[0] <= 3 and want.idx[2] <= 7 and want.mult[0] >= 2 and want.mult[2] >= 2
    assert (want.idx >= 512).sum() > 10 and ((want.idx >= 0) & (want.idx < 512)).sum() > 10 and (want.idx < 0).sum() > 10
    B = dev.DMat.wrap(t.data_ptr() + 8 * 6, n, ncols, ld, keep=t)
    dev.copy_block(B, 0, 0, dev.DMat.from_words(bw, ncols), 0, 0, n, ncols)
    A = dev.DMat.from_words(aw, ncols)
    idx, mult, count = dev.find_rows(A, B, c0, c1)
    assert np.array_equal(idx.read(None), want.idx) and np.array_equal(mult.read(None), want.mult)
    assert int(count.read(None)[0]) == want.count
    del t, B
    gc.collect()
    torch.cuda.empty_cache()


# ---- reproducibility, wrappers -----------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits(dev):
    n, ncols = 20000, 256
    a, b, _ = pools(n, n, ncols, 0, ncols, 3)
    A, B = dev.DMat.from_words(to_words(a, ncols), ncols), dev.DMat.from_words(to_words(b, ncols), ncols)
    results = []
    for _ in range(2):
        idx, mult, count = dev.find_rows(A, B)
        results.append((idx.read(None), mult.read(None), count.read(None)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert 0 < int(results[0][2][0]) < n and results[0][1].max() > 1


def test_the_wrappers(dev):
    na, nb, ncols, c0, c1 = 6000, 5000, 300, 40, 260
    a, b, _ = pools(na, nb, ncols, c0, c1, 8)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    want = fr.find_rows(aw, bw, c0, c1)
    A, B = dev.DMat.from_words(aw, ncols), dev.DMat.from_words(bw, ncols)
    idx = A.find_in(B, c0, c1)
    assert np.array_equal(idx.read(None), want.idx)
    miss, hit = A.difference(B, c0, c1), A.intersection(B, c0, c1)
    assert (miss.nrows, miss.ncols) == (na - want.count, ncols) and (hit.nrows, hit.ncols) == (want.count, ncols)
    assert np.array_equal(miss.to_words(), aw[want.idx < 0]) and np.array_equal(hit.to_words(), aw[want.idx >= 0])   # in their order
    assert miss.nrows + hit.nrows == na and 0 < hit.nrows < na                   # together they partition A
    # gather_rows(B, idx): A's range bits for the hits, zero rows for the misses
    D, bad = dev.gather_rows(B, idx.ptr, D=dev.DMat(na, ncols), bad=None)
    got = D.to_words()
    assert bad is False and not got[want.idx < 0].any()
    assert np.array_equal(ur.range_words(got[want.idx >= 0], c0, c1), ur.range_words(aw[want.idx >= 0], c0, c1))
    # the whole row of the narrower matrix is the default range
    whole = fr.find_rows(aw, bw, 0, ncols)
    assert np.array_equal(A.find_in(B).read(None), whole.idx) and A.intersection(B).nrows == whole.count
    idx, mult, count = dev.find_rows(A, B, c0, c1, mult=dev.SKIP, count=dev.SKIP)
    assert mult is None and count is None and np.array_equal(idx.read(None), want.idx)
    # empty A and empty B
    E = dev.DMat(0, ncols)
    idx, mult, count = dev.find_rows(E, B, c0, c1)
    assert int(count.read(None)[0]) == 0 and idx is not None and mult is not None
    assert (E.difference(B).nrows, E.intersection(B).nrows, E.difference(B).ncols) == (0, 0, ncols)
    idx, mult, count = dev.find_rows(A, E, c0, c1)
    assert (idx.read(None) == -1).all() and not mult.read(None).any() and int(count.read(None)[0]) == 0 and len(idx.read(None)) == na
    assert A.intersection(E, c0, c1).nrows == 0 and np.array_equal(A.difference(E, c0, c1).to_words(), aw)
    assert A.difference(A).nrows == 0 and np.array_equal(A.intersection(A).to_words(), aw)
    with pytest.raises(ValueError):
        dev.find_rows(A, B, idx=dev.SKIP)
    with pytest.raises(Exception, match="columns"):
        dev.find_rows(A, B, 5, 4)
    assert np.array_equal(A.to_words(), aw) and np.array_equal(B.to_words(), bw)


# ---- census ------------------------------------------------------------------------------------------------------------------------

def test_every_kernel_of_the_module_is_launched(dev, L):
    """each kernel of gf2_find.hip, and every instance of it, by name: one call on the lane form and one on the wave form"""
    k0 = census(L)
    for ncols, c0, c1 in ((130, 1, 129), (1000, 3, 997)):
        words = pool(2500, ncols, c0, c1, 4)
        P = dev.DMat.from_words(words, ncols)
        dev.find_rows(P, P, c0, c1)
    k1 = census(L)
    for name in [FILL, BUILD[0], BUILD[1], LOOKUP[0], LOOKUP[1]]:
        assert launches(k0, k1, name) == (2 if name == FILL else 1), name
    assert launches(k0, k1, "gf2_find_") == 6
