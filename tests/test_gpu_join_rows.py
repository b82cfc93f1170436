"""GPU tests of include/m4ri_hip_join_rows.h: gf2_group_rows_dev and gf2_join_rows_dev bit for bit against the numpy yardstick of
tests/join_rows_ref.py (itself checked against a double loop by tests/test_join_rows_reference.py) and, on the device, against the
entries the header names: gf2_join_dev, gf2_near_pairs_dev, gf2_unique_rows_dev, gf2_find_rows_dev and gf2_sort_rows_dev.

The harness is that of tests/test_gpu_find.py: A, B and D are windows of dirty parents (View of tests/test_gpu_lf1.py: the excess bits
of the last word are dirty too) in the four layouts EE / EO / OE / OO, and the parents are compared afterwards -- A and B unchanged, D
changed in the rows below min(count, capacity) alone; the int outputs lie between sentinels and hold a pattern before the call; which
kernels ran, and how many launches a call took, is read from the launch census and compared with gf2_join_rows_plan.

The pools are those of tests/test_gpu_find.py (pools()): classes of several members scattered through B; for every column of the range
a row of A that differs from a row of B in that column alone, which must not match; a row that agrees on the range and differs at
c0 - 1 and c1, which must."""
import gc

import numpy as np
import pytest

import join_rows_ref as jr
from census_util import assert_route, census
from stream_util import SLEEP_CYCLES
from test_gpu_find import launches, pools, to_words
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded
from test_gpu_unique import pool, with_values

pytestmark = pytest.mark.gpu

BIG_A, BIG_B = 3 * 4096 + 5, 2 * 4096 + 3
LAYOUTS4 = [EE, EO, OE, OO]
PAIRS, STARTS, HEADS = "gf2_join_rows_pairs_kernel", "gf2_join_rows_starts_kernel", "gf2_join_rows_heads_kernel"
SUMS, SCAN, OFFSETS = "gf2_join_rows_sums_kernel", "gf2_join_rows_scan_kernel", "gf2_join_rows_offsets_kernel"
SCATTER = {lanes: "gf2_join_rows_scatter_kernelILi%dEE" % lanes for lanes in (1, 2, 8, 64)}
BUILD = {0: "gf2_find_build_kernelILb0EE", 1: "gf2_find_build_kernelILb1EE"}
OWN = "gf2_join_rows_"


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


def lanes_of(ncols):
    nw = (ncols + 63) // 64
    return 1 if nw <= 2 else 2 if nw <= 4 else 8 if nw <= 64 else 64


def guarded64():
    """one device int64 between sentinels -> (tensor, address)"""
    import torch
    t = torch.full((4,), 0x5EAD5EAD5EAD5EAD, dtype=torch.int64, device="cuda")
    return t, t.data_ptr() + 16


def read_count(t):
    h = t.cpu().numpy()
    assert h[0] == h[1] == h[3] == 0x5EAD5EAD5EAD5EAD, "a word next to the count was written"
    return int(h[2])


def run_group(dev, L, words, ncols, c0, c1, layout=EE, head=True, stream=None):
    """gf2_group_rows_dev on a dirty window against the yardstick -> (order, head) of the yardstick"""
    import torch
    n = len(words)
    want = jr.group_rows(words, c0, c1)
    P = View(dev, n, ncols, layout, 3 * n + c1, words)
    (to, po), (th, ph) = guarded(n), guarded(n)
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.group_rows(P.m, c0, c1, order=po, head=ph if head else dev.SKIP, stream=stream)
    assert out == (None, None)
    torch.cuda.synchronize()
    k1 = census(L)
    what = (n, ncols, c0, c1, layout, head)
    assert np.array_equal(read_guarded(to), want[0]), what
    assert np.array_equal(read_guarded(th), want[1] if head else np.full(n, SENT)), what
    P.unchanged()
    plan = dev.join_rows_plan(0, n, ncols, c0, c1)
    assert launches(k0, k1) == (plan[3] + (2 if head else 0) if n else 0), (what, launches(k0, k1), plan)
    if n:
        assert launches(k0, k1, "gf2_find_") == 3 and launches(k0, k1, BUILD[plan[2]]) == 1, what
        assert launches(k0, k1, "gf2_lf2_sort_scatter_kernel") == plan[0] == ((n - 1).bit_length() + 7) // 8, what
        assert launches(k0, k1, PAIRS) == (1 if n > 1 else 0) and launches(k0, k1, "gf2_lf2_iota") == (1 if n == 1 else 0), what
        assert launches(k0, k1, STARTS) == launches(k0, k1, HEADS) == int(head), what
    return want


def run_join(dev, L, aw, bw, ncols, c0, c1, wcols=None, cap="equal", la=EE, lb=OO, ld=EO, store=True, arrays=(True, True, True),
             stream=None, want=None, a_is_b=False):
    """gf2_join_rows_dev on dirty windows against the yardstick -> the yardstick's result for ALL pairs"""
    import torch
    na, nb = len(aw), len(bw)
    wc0, wc1 = (0, ncols) if wcols is None else wcols
    if want is None:
        want = jr.join_rows(aw, bw, ncols, c0, c1, wc0, wc1)
    capn = {"zero": 0, "one": 1, "less": max(want.count - 1, 0), "equal": want.count, "more": want.count + 5}[cap] if isinstance(cap, str) else cap
    m = min(capn, want.count)
    A = View(dev, na, ncols, la, 5 * na + c0, aw)
    B = A if a_is_b else View(dev, nb, ncols, lb, 7 * nb + c1, bw)
    D = View(dev, capn, ncols, ld, 11 * capn + 1) if store else None
    Dm = D.m if store else dev.DMat.wrap(None, capn, ncols, max((ncols + 63) // 64, 1))
    (ta, pa), (tb, pb), (tw, pw), (tc, pc) = guarded(capn), guarded(capn), guarded(capn), guarded64()
    ptrs = [p if on else None for p, on in zip((pa, pb, pw), arrays)]
    torch.cuda.synchronize()
    k0 = census(L)
    rc = L.gf2_join_rows_dev(Dm._on(stream), A.m._on(stream), B.m._on(stream), c0, c1, pc, ptrs[0], ptrs[1], ptrs[2], wc0, wc1, stream)
    assert rc == 0, L.gf2_last_error()
    torch.cuda.synchronize()
    k1 = census(L)
    what = (na, nb, ncols, c0, c1, wcols, capn, la, lb, ld, store, arrays)
    assert read_count(tc) == want.count, (what, read_count(tc), want.count)
    for t, ref, on in ((ta, want.ia, arrays[0]), (tb, want.ib, arrays[1]), (tw, want.wt, arrays[2])):
        got = read_guarded(t)
        assert np.array_equal(got[:m], ref[:m] if on else np.full(m, SENT)), (what, np.flatnonzero(got[:m] != ref[:m])[:8])
        assert np.all(got[m:] == SENT), (what, "an entry behind min(count, capacity) was written")
    A.unchanged()
    B.unchanged()
    if store:                                             # whole rows below min(count, capacity), the excess bits zero, nothing else
        assert np.array_equal(D.read(), D.with_rows(want.d[:m])), (what, "D")
    plan = dev.join_rows_plan(na, nb, ncols, c0, c1)
    writes = capn > 0 and ((store and ncols > 0) or any(arrays))
    expect = 0 if not (na and nb) else plan[4] if writes else 5
    assert launches(k0, k1) == expect, (what, launches(k0, k1), plan)
    if na and nb:
        assert_route(k0, k1, [BUILD[plan[2]], SUMS, SCAN])
        assert launches(k0, k1, "gf2_find_") == (6 if writes else 3) and launches(k0, k1, BUILD[1 - plan[2]]) == 0, what
        assert launches(k0, k1, OWN) == (2 + (1 + (1 if nb > 1 else 0) + 1 + 1 if writes else 0)), what
        if writes:
            assert launches(k0, k1, SCATTER[lanes_of(ncols)]) == 1 and launches(k0, k1, "gf2_lf2_sort_scatter_kernel") == plan[0], what
    return want


# ---- row counts --------------------------------------------------------------------------------------------------------------------

def test_the_sizes_are_the_plans(dev):
    assert dev.join_rows_plan(1000, 1000, 200, 57, 200)[5:7] == (1024, 2048) and dev.join_rows_plan(1000, 1000, 704, 3, 700)[2] == 1
    assert [lanes_of(n) for n in (100, 200, 704, 4200)] == [1, 2, 8, 64]


SIZES = [0, 1, 63, 64, 65, 257]
COUNTS = [(n, n) for n in SIZES] + [(0, 64), (64, 0), (1, 257), (257, 1), (63, 65), (65, 64), (BIG_A, BIG_B)]


@pytest.mark.parametrize("sizes", COUNTS, ids=lambda s: "%dx%d" % s)
def test_row_counts(dev, L, sizes):
    na, nb = sizes
    ncols, c0, c1 = 200, 37, 82
    a, b, _ = pools(na, nb, ncols, c0, c1, 100 + na + 3 * nb)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    k = na % 4
    want = run_join(dev, L, aw, bw, ncols, c0, c1, wcols=(30, 90), la=LAYOUTS4[k], lb=LAYOUTS4[nb % 4], ld=LAYOUTS4[(k + 2) % 4])
    if na >= 63 and nb >= 63:
        assert want.count > na // 4 and len(set(want.ia.tolist())) < na       # classes of several members, and rows without a partner
    if na == BIG_A:
        assert want.count > 3 * 2048 and dev.join_rows_plan(na, nb, ncols, c0, c1)[0] == 2   # several chunks, runs and sort tiles
    if not (na and nb):
        assert want.count == 0
    run_group(dev, L, bw, ncols, c0, c1, layout=LAYOUTS4[(nb + 1) % 4])


# ---- ranges ------------------------------------------------------------------------------------------------------------------------

RANGES = [(200, 0, 0), (200, 5, 35), (200, 37, 82), (200, 64, 128), (200, 0, 200), (704, 3, 700), (100, 20, 90), (4200, 100, 4190)]
WEIGHTS = {"empty": lambda n, c0, c1: (c0, c0), "inside": lambda n, c0, c1: (c0 + (c1 - c0) // 4, c1 - (c1 - c0) // 4),
           "straddling": lambda n, c0, c1: (max(c0 - 9, 0) if c0 else 0, min(c0 + (c1 - c0) // 2 + 70, n))}


@pytest.mark.parametrize("weights", sorted(WEIGHTS))
@pytest.mark.parametrize("case", RANGES, ids=lambda c: "%d-c%d-%d" % c)
def test_ranges(dev, L, case, weights):
    """the empty range, 30 bits, a range that crosses a word at an odd offset, a word-aligned one, the whole row, 11 words (the wave
    form of the table), and rows of 2 and 66 words (1 and 64 lanes per row of the scatter); every weight range on each"""
    ncols, c0, c1 = case
    na, nb = (150, 130) if c0 == c1 else (1500, 1300) if ncols < 4000 else (400, 300)
    a, b, src = pools(na, nb, ncols, c0, c1, 7 * ncols + c0)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    k = RANGES.index(case) + sorted(WEIGHTS).index(weights)
    wcols = WEIGHTS[weights](ncols, c0, c1)
    want = run_join(dev, L, aw, bw, ncols, c0, c1, wcols=wcols, la=LAYOUTS4[k % 4], lb=LAYOUTS4[(k + 1) % 4], ld=LAYOUTS4[(k + 3) % 4])
    assert dev.join_rows_plan(na, nb, ncols, c0, c1)[2] == (1 if c1 - c0 > 600 else 0)
    if c0 == c1:
        assert want.count == na * nb
        return
    outside = weights == "straddling" and (wcols[0] < c0 or wcols[1] > c1)        # the whole row leaves nothing outside
    assert want.wt.max() > 0 if outside else not want.wt.any()                 # partners agree inside the range: no ones there
    # what the pools promise, read off the yardstick: partners agree on the range ...
    assert np.array_equal(a[want.ia, c0:c1], b[want.ib, c0:c1]) and set(range(0, na, 2)) <= set(want.ia.tolist())
    planted = np.arange(1, na, 2)[:min(c1 - c0, na // 4)]
    partners = {(i, j) for i, j in zip(want.ia.tolist(), want.ib.tolist())}
    assert not any((i, src[i]) in partners for i in planted.tolist())          # ... one flipped column is no match ...
    i = (na - 1) & ~1                                                           # ... and the columns next to the range do not count
    assert (i, src[i]) in partners
    if c0 > 0 and c1 < ncols:
        assert a[i, c0 - 1] != b[src[i], c0 - 1] and a[i, c1] != b[src[i], c1]


@pytest.mark.parametrize("case", RANGES[:6], ids=lambda c: "%d-c%d-%d" % c)
def test_group_ranges(dev, L, case):
    ncols, c0, c1 = case
    for n, head in ((5000, True), (300, False)):
        want = run_group(dev, L, pool(n, ncols, c0, c1, n + c1), ncols, c0, c1, layout=LAYOUTS4[RANGES.index(case) % 4], head=head)
        if c0 == c1:
            assert np.array_equal(want[0], np.arange(n)) and not want[1].any()
        else:
            assert n // 4 < len(set(want[1].tolist())) < n


# ---- skew --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["b-all-equal", "all-distinct", "disjoint", "a-is-b", "sparse-hits"])
def test_class_shapes(dev, L, shape):
    ncols, c0, c1 = 200, 37, 82
    rng = np.random.default_rng(len(shape))
    if shape == "b-all-equal":                                                  # every row of A owns 1500 outputs: most of a chunk each
        na, nb = 70, 1500
        ids_a, ids_b = np.zeros(na, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    elif shape == "all-distinct":
        na, nb = 5000, 5000
        ids_b, ids_a = rng.permutation(nb), rng.integers(0, 2 * nb, na)
    elif shape == "disjoint":
        na, nb = 3000, 3000
        ids_b, ids_a = rng.permutation(nb), nb + rng.integers(0, nb, na)
    elif shape == "a-is-b":
        na = nb = 5000
        ids_a = ids_b = rng.integers(0, nb // 3, nb)
    else:                                                                       # two hits 9000 rows apart: the stretch is bisected in global memory
        na, nb = 9500, 600
        ids_b = rng.integers(0, 100, nb)
        ids_a = 1000 + np.arange(na)
        ids_a[[200, 9300]] = 7
    ids = np.concatenate([ids_b, ids_a]) if shape != "a-is-b" else ids_b
    words = with_values(len(ids), ncols, c0, c1, 31 + len(shape), ids)
    bw, aw = words[:nb], (words[nb:] if shape != "a-is-b" else words)
    want = run_join(dev, L, aw, bw, ncols, c0, c1, wcols=(0, 100), la=OO, lb=EO, ld=OE, a_is_b=shape == "a-is-b")
    members = {}
    for j, v in enumerate(ids_b.tolist()):
        members.setdefault(v, []).append(j)
    expect = [(i, j) for i, v in enumerate(ids_a.tolist()) for j in members.get(v, [])]   # the ids say the same as the yardstick
    assert list(zip(want.ia.tolist(), want.ib.tolist())) == expect
    if shape == "b-all-equal":
        assert want.count == 70 * 1500 and np.array_equal(want.ib, np.tile(np.arange(1500), 70))
    elif shape == "all-distinct":
        assert 0 < want.count < na and len(set(want.ia.tolist())) == want.count
    elif shape == "disjoint":
        assert want.count == 0
    elif shape == "a-is-b":
        assert want.count > na and (want.ia == want.ib).sum() == na            # all ordered pairs of a class, (i, i) included
    else:
        assert set(want.ia.tolist()) == {200, 9300} and want.count == 2 * len(members[7])


# ---- capacity, index-only, NULL arrays ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", ["equal", "less", "one", "zero", "more", 2048, 2049])
def test_capacity(dev, L, cap):
    ncols, c0, c1 = 200, 64, 128
    a, b, _ = pools(3000, 2500, ncols, c0, c1, 55)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    want = run_join(dev, L, aw, bw, ncols, c0, c1, wcols=(60, 130), cap=cap, la=EO, lb=OE, ld=OO)
    assert want.count > 2 * 2048


@pytest.mark.parametrize("case", [(200, 64, 128), (704, 3, 700)], ids=lambda c: "%d-c%d-%d" % c)
def test_index_only_and_null_arrays(dev, L, case):
    """D->data == NULL: the arrays alone, each of them NULL in turn, and with all three NULL nothing but the count; then the same
    arrays with D stored: a skipped array keeps its pattern and the launches stay the plan's (run_join holds both)"""
    ncols, c0, c1 = case
    a, b, _ = pools(1200, 1100, ncols, c0, c1, 56)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    want = jr.join_rows(aw, bw, ncols, c0, c1, 10, ncols - 10)
    for arrays in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        for store in (False, True):
            run_join(dev, L, aw, bw, ncols, c0, c1, wcols=(10, ncols - 10), cap="more", store=store, arrays=arrays, want=want, la=OE, lb=EE, ld=EO)
    run_join(dev, L, aw, bw, ncols, c0, c1, wcols=(10, 10), cap="less", store=False, want=jr.join_rows(aw, bw, ncols, c0, c1, 10, 10))


# ---- a count past 2^31 -------------------------------------------------------------------------------------------------------------

def test_a_count_of_2_to_32(dev, L):
    """65536 rows a side, all equal on [0, 64): the count-only call gives exactly 2^32; a capacity of 1000 gives row 0 of A with the
    rows 0 .. 999 of B, and nothing behind entry 999 is written"""
    import torch
    n, ncols = 65536, 128
    rng = np.random.default_rng(64)
    aw, bw = (rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64) for _ in range(2))
    aw[:, 0] = bw[:, 0] = np.uint64(0x0123456789ABCDEF)
    A, B = dev.DMat.from_words(aw, ncols), dev.DMat.from_words(bw, ncols)
    tc, pc = guarded64()
    D, count, ia, ib, wt = dev.join_rows(A, B, 0, 64, cap=0, count=pc)
    torch.cuda.synchronize()
    assert read_count(tc) == 1 << 32 and D.nrows == 0
    cap = 1000
    (ta, pa), (tb, pb), (tw, pw) = guarded(cap + 50), guarded(cap + 50), guarded(cap + 50)
    Dv = View(dev, cap + 3, ncols, OO, 65)
    Dm = dev.DMat.wrap(Dv.m.s.data, cap, ncols, Dv.m.ld, keep=Dv.t)
    dev.join_rows(A, B, 0, 64, D=Dm, count=pc, ia=pa, ib=pb, wt=pw, wcols=(64, 128))
    torch.cuda.synchronize()
    assert read_count(tc) == 1 << 32
    d = aw[:1] ^ bw[:cap]
    for t, ref in ((ta, np.zeros(cap)), (tb, np.arange(cap)), (tw, jr.weights(d, ncols, 64, 128))):
        got = read_guarded(t)
        assert np.array_equal(got[:cap], ref) and np.all(got[cap:] == SENT)
    assert np.array_equal(Dv.read(), Dv.with_rows(d))                          # the three rows behind the capacity keep their junk


# ---- equivalences on the device ----------------------------------------------------------------------------------------------------

def test_a_narrow_range_is_the_join_on_a_window_reordered(dev):
    """(a): c1 - c0 <= 30"""
    ncols, c0, c1 = 200, 5, 35
    a, b, _ = pools(4000, 3500, ncols, c0, c1, 71)
    A, B = dev.DMat.from_words(to_words(a, ncols), ncols), dev.DMat.from_words(to_words(b, ncols), ncols)
    D, count, ia, ib, wt = dev.join_rows(A, B, c0, c1, wcols=(3, 150))
    D2, count2, ia2, ib2, wt2 = dev.join(A, B, c0, c1 - c0, wcols=(3, 150))
    n = int(count.read(None)[0])
    assert n == int(count2.read(None)[0]) == D.nrows == D2.nrows and n > 2048
    x, y = ia2.read(None), ib2.read(None)
    by = np.lexsort([y, x])                                                     # the window join's pairs, by (ia, ib)
    assert not np.array_equal(by, np.arange(n))                                 # its own order is by key
    assert np.array_equal(ia.read(None), x[by]) and np.array_equal(ib.read(None), y[by]) and np.array_equal(wt.read(None), wt2.read(None)[by])
    assert np.array_equal(D.to_words(), D2.to_words()[by])


def test_an_empty_range_is_the_all_pairs_search(dev):
    """(b): c0 == c1 against gf2_near_pairs_dev with flags == 0, wlo = 0, whi = ncols, bit for bit"""
    ncols = 200
    a, b, _ = pools(70, 90, ncols, 50, 50, 72)
    A, B = dev.DMat.from_words(to_words(a, ncols), ncols), dev.DMat.from_words(to_words(b, ncols), ncols)
    D, count, ia, ib, wt = dev.join_rows(A, B, 50, 50, wcols=(13, 177))
    D2, hits, ia2, ib2, wt2 = dev.near_pairs(A, B, (13, 177), 0, ncols)
    assert int(count.read(None)[0]) == int(hits.read(None)[0]) == 70 * 90 == D.nrows == D2.nrows
    for x, y in ((ia, ia2), (ib, ib2), (wt, wt2)):
        assert np.array_equal(x.read(None), y.read(None))
    assert np.array_equal(D.to_words(), D2.to_words())


@pytest.mark.parametrize("case", [(200, 37, 82), (704, 3, 700)], ids=lambda c: "%d-c%d-%d" % c)
def test_the_grouping_against_unique_find_and_the_join(dev, case):
    """order[head[s]] is the rep of gf2_unique_rows_dev, the class sizes are the mult of gf2_find_rows_dev, the classes are those of
    gf2_sort_rows_dev, and (c): with A == B the partners of the lowest row of a class are the class in the grouping's order"""
    ncols, c0, c1 = case
    n = BIG_B
    P = dev.DMat.from_words(pool(n, ncols, c0, c1, n + c1), ncols)
    order, head = (x.read(None) for x in dev.group_rows(P, c0, c1))
    rep = dev.unique_rows(P, c0, c1, cap=n)[2].read(None)
    mult = dev.find_rows(P, P, c0, c1)[1].read(None)
    assert sorted(order.tolist()) == list(range(n)) and np.array_equal(order[head], rep[order])
    starts = np.flatnonzero(head == np.arange(n))
    sizes = np.diff(np.r_[starts, n])
    assert np.array_equal(np.repeat(sizes, sizes), mult[order]) and sizes.max() > 1
    assert np.all(np.diff(order[starts]) > 0)                                   # the classes by their lowest row
    sorder, shead = (x.read(None) for x in dev.sort_rows(P, c0, c1))
    assert {tuple(c.tolist()) for c in np.split(sorder, np.flatnonzero(np.diff(shead)) + 1)} == \
        {tuple(c.tolist()) for c in np.split(order, starts[1:])}
    D, count, ia, ib, wt = dev.join_rows(P, P, c0, c1, store=False, wt=dev.SKIP)
    ia, ib = ia.read(None), ib.read(None)
    assert D is None and int(count.read(None)[0]) == int((sizes.astype(np.int64) ** 2).sum()) == len(ia)
    lowest = np.isin(ia, order[starts]) & (rep[ia] == ia)
    assert np.array_equal(ib[lowest], order)                                    # class after class, by lowest row: the whole order


# ---- streams, dirty scratch, determinism -------------------------------------------------------------------------------------------

def test_behind_pending_work_on_a_caller_stream(dev, L):
    """A and B are gathered from a seeded dictionary on the caller's stream, behind a sleep; join and grouping are enqueued twice
    behind it, into two sets of outputs, before anything synchronises"""
    import limits_ref as lr
    import torch
    n, ncols, seed, c0, c1 = 6001, 200, 0x51DF, 10, 190
    known = n // 3
    dictionary = lr.seeded_words(seed, ncols, np.arange(2 * known))
    rng = np.random.default_rng(6)
    jb, ja = rng.integers(0, known, n).astype(np.int32), rng.integers(0, 2 * known, n).astype(np.int32)
    want = jr.join_rows(dictionary[ja], dictionary[jb], ncols, c0, c1, 0, 64)
    worder, whead = jr.group_rows(dictionary[jb], c0, c1)
    assert want.count > n
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    td = torch.full((2 * known, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ta, tb = (torch.full((n, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda") for _ in range(2))
    tja, tjb = torch.from_numpy(ja).cuda(), torch.from_numpy(jb).cuda()
    S, A, B = dev.DMat.from_torch(td, ncols), dev.DMat.from_torch(ta, ncols), dev.DMat.from_torch(tb, ncols)
    cap = want.count + 9
    outs = [[guarded(cap), guarded(cap), guarded(cap), guarded64(), guarded(n), guarded(n), dev.DMat(cap, ncols)] for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(SLEEP_CYCLES)
    S.fill_random(seed, s)
    dev.gather_rows(S, tja.data_ptr(), D=A, stream=s)
    dev.gather_rows(S, tjb.data_ptr(), D=B, stream=s)
    for (_, pa), (_, pb), (_, pw), (_, pc), (_, po), (_, ph), D in outs:
        dev.join_rows(A, B, c0, c1, D=D, count=pc, ia=pa, ib=pb, wt=pw, wcols=(0, 64), stream=s)
        dev.group_rows(B, c0, c1, order=po, head=ph, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for (ta_, _), (tb_, _), (tw_, _), (tc_, _), (to_, _), (th_, _), D in outs:
        m = want.count
        assert read_count(tc_) == m
        for t, ref in ((ta_, want.ia), (tb_, want.ib), (tw_, want.wt)):
            assert np.array_equal(read_guarded(t)[:m], ref) and np.all(read_guarded(t)[m:] == SENT)
        assert np.array_equal(D.to_words()[:m], want.d)
        assert np.array_equal(read_guarded(to_), worder) and np.array_equal(read_guarded(th_), whead)


def test_on_dirty_scratch(dev, L):
    """the scratch comes from a cache in which every block holds a pattern, and no block comes fresh from the driver: a table entry,
    a class start or an offset that the call did not write would be read"""
    import dirty_pool as dp
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for na, nb, ncols, c0, c1 in ((BIG_A, BIG_B, 200, 37, 82), (3000, 2600, 704, 3, 700)):
            a, b, _ = pools(na, nb, ncols, c0, c1, na)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run_join(dev, L, to_words(a, ncols), to_words(b, ncols), ncols, c0, c1, wcols=(1, 99), stream=stream, la=OE, lb=EE, ld=OO)
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the wide join on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_two_calls_give_the_same_bits(dev):
    n, ncols = 20000, 256
    a, b, _ = pools(n, n, ncols, 0, ncols, 3)
    A, B = dev.DMat.from_words(to_words(a, ncols), ncols), dev.DMat.from_words(to_words(b, ncols), ncols)
    results = []
    for _ in range(2):
        D, count, ia, ib, wt = dev.join_rows(A, B, wcols=(100, 200))
        order, head = dev.group_rows(B)
        results.append((D.to_words(), count.read(None), ia.read(None), ib.read(None), wt.read(None), order.read(None), head.read(None)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert int(results[0][1][0]) > n // 2 and results[0][0].shape[0] == int(results[0][1][0])


# ---- wrappers ----------------------------------------------------------------------------------------------------------------------

def test_the_wrappers(dev):
    na, nb, ncols, c0, c1 = 3000, 2500, 300, 40, 260
    a, b, _ = pools(na, nb, ncols, c0, c1, 8)
    aw, bw = to_words(a, ncols), to_words(b, ncols)
    want = jr.join_rows(aw, bw, ncols, c0, c1, 5, 280)
    A, B = dev.DMat.from_words(aw, ncols), dev.DMat.from_words(bw, ncols)
    D = A.join_rows(B, c0, c1)                                                  # count first: exactly `count` rows
    assert (D.nrows, D.ncols) == (want.count, ncols) and np.array_equal(D.to_words(), want.d)
    D, wt = A.join_rows(B, c0, c1, wcols=(5, 280))
    assert np.array_equal(D.to_words(), want.d) and np.array_equal(wt.read(None), want.wt)
    assert np.array_equal(B.group_rows(c0, c1).read(None), jr.group_rows(bw, c0, c1)[0])
    whole = jr.join_rows(aw, bw, ncols, 0, ncols)                               # the whole row is the default range
    assert A.join_rows(B).nrows == whole.count
    D, count, ia, ib, wt = dev.join_rows(A, B, c0, c1, store=False, wcols=(5, 280))
    assert D is None and np.array_equal(ia.read(None), want.ia) and np.array_equal(ib.read(None), want.ib) and np.array_equal(wt.read(None), want.wt)
    D, count, ia, ib, wt = dev.join_rows(A, B, c0, c1, cap=10, ia=dev.SKIP, wt=dev.SKIP)
    assert D.nrows == 10 and ia is None and wt is None and np.array_equal(ib.read(None), want.ib[:10]) and int(count.read(None)[0]) == want.count
    # the join's arrays feed the gathers
    D, count, ia, ib, wt = dev.join_rows(A, B, c0, c1)
    Ga, Gb = dev.gather_rows(A, ia.ptr, D=dev.DMat(want.count, ncols))[0], dev.gather_rows(B, ib.ptr, D=dev.DMat(want.count, ncols))[0]
    assert np.array_equal(Ga.to_words() ^ Gb.to_words(), D.to_words())
    # empty A and empty B
    E = dev.DMat(0, ncols)
    for X, Y in ((E, B), (A, E), (E, E)):
        D, count, ia, ib, wt = dev.join_rows(X, Y, c0, c1)
        assert D.nrows == 0 and int(count.read(None)[0]) == 0
    assert len(E.group_rows().read(None)) == 0
    with pytest.raises(Exception, match="columns"):
        dev.join_rows(A, B, 5, 4, cap=1)
    assert np.array_equal(A.to_words(), aw) and np.array_equal(B.to_words(), bw)


# ---- census ------------------------------------------------------------------------------------------------------------------------

def test_every_kernel_of_the_module_is_launched(dev, L):
    """each kernel of gf2_join_rows.hip, and every instance of the scatter, by name: a join on each row width class and a grouping
    with head"""
    k0 = census(L)
    for ncols in (100, 200, 704, 4200):
        words = pool(300, ncols, 3, 90, ncols)
        P = dev.DMat.from_words(words, ncols)
        dev.join_rows(P, P, 3, 90, cap=50)
    dev.group_rows(P, 3, 90)
    k1 = census(L)
    for lanes in (1, 2, 8, 64):
        assert launches(k0, k1, SCATTER[lanes]) == 1, lanes
    for name, times in ((PAIRS, 5), (STARTS, 5), (HEADS, 1), (SUMS, 4), (SCAN, 4), (OFFSETS, 4)):
        assert launches(k0, k1, name) == times, name
    assert launches(k0, k1, OWN) == 4 + 5 + 5 + 1 + 12
