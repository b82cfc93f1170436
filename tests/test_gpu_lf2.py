"""GPU tests of include/m4ri_hip_lf2.h: gf2_class_sort_dev and gf2_lf2_reduce_dev bit for bit against the numpy yardstick of
tests/lf2_ref.py (itself checked against the definition by tests/test_lf2_reference.py): the rows of D that are written, the rest of
D, the words around D, `count`, `lo` and `hi` up to min(count, capacity), `order` and `skeys` in full.

Every operand is a window of a dirty parent (View of tests/test_gpu_lf1.py): random bits in every word of the parent -- the rows
before and behind the window, the words left and right of it, the excess bits of P's last word -- and the whole parent of D is
compared afterwards.  The int outputs lie between sentinels and hold a pattern before the call.

T (rows of a sort tile), R (sorted positions of a run of the pair kernels), the passes and the lanes per row are read from
gf2_lf2_plan, never written down here; which kernels ran is read from the launch census."""
import gc

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import lf1_ref as l1
import lf2_ref as lf
import limits_ref as lr
from census_util import assert_route, census
from test_gpu_lf1 import EE, EO, LAYOUT_PAIRS, OE, OO, SENT, View, guarded, read_guarded, set_keys

pytestmark = pytest.mark.gpu


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


def plan_of():
    try:
        from m4ri_rust_amd import device
        p = device.lf2_plan(1000, 256, 8)
        return p[4], p[5]
    except Exception:   # not built yet: the fixture builds; test_the_cases_are_the_plans checks the sizes
        return 4096, 1024


T, R = plan_of()


def test_the_cases_are_the_plans(dev):
    assert (T, R) == plan_of() == dev.lf2_plan(5, 64, 30)[4:6] and T > R >= 256
    assert [dev.lf2_plan(10, 64, b)[0] for b in (0, 1, 8, 9, 16, 17, 24, 25, 30)] == [0, 1, 1, 2, 2, 3, 3, 4, 4]


def keyed(N, ncols, c0, b, k, seed):
    """N random rows whose keys are k"""
    return set_keys(g.random_words(N, ncols, seed), c0, b, k)


def drawn(N, b, classes, seed):
    """N keys drawn from `classes` random values below 2^b"""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 1 << b, max(classes, 1))
    return values[rng.integers(0, len(values), N)]


def sort_families(b):
    if b == 0:
        return ["gf2_lf2_iota_kernel"]
    return ["gf2_lf2_sort_count_kernel", "gf2_lf2_scan_sums_kernel", "gf2_lf2_scan_group_kernelIi", "gf2_lf2_scan_apply_kernel",
            "gf2_lf2_sort_scatter_kernel"]


def capacity(cap, count):
    return {"zero": 0, "less": count // 2, "equal": count, "more": count + 7}[cap] if isinstance(cap, str) else cap


def count_of(t):
    return int(read_guarded(t)[:2].copy().view(np.int64)[0])


def run(dev, L, words, ncols, c0, b, cap="more", lo=True, hi=True, layouts=(EE, EE), stream=None):
    """one gf2_lf2_reduce_dev call on dirty windows against the yardstick -> (count, the yardstick's rows that were written)"""
    import torch
    N = words.shape[0]
    count = lf.pair_count(lf.keys(words, c0, b))
    capn = capacity(cap, count)
    n = min(count, capn)
    want = lf.lf2(words, ncols, c0, b, limit=n)
    assert want.count == count and len(want.lo) == n
    P = View(dev, N, ncols, layouts[0], 11 * N + c0, words)
    D = View(dev, capn, ncols, layouts[1], 13 * N + b) if capn else None
    Dm = D.m if D else dev.DMat.wrap(None, 0, ncols, g.width(ncols))
    tc, pc = guarded(2)
    tl, pl = guarded(max(capn, 1))
    th, ph = guarded(max(capn, 1))
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.lf2_reduce(P.m, c0, b, D=Dm, count=pc, lo=pl if lo and capn else dev.SKIP, hi=ph if hi and capn else dev.SKIP, stream=stream)
    assert out[0] is Dm and out[1:] == (None, None, None)
    torch.cuda.synchronize()
    what = (N, ncols, c0, b, cap, layouts)
    assert count_of(tc) == count, what
    for t, given, rows in ((tl, lo, want.lo), (th, hi, want.hi)):
        a = read_guarded(t)
        if given and capn:
            assert np.array_equal(a[:n], rows), (what, np.flatnonzero(a[:n] != rows)[:8])
        assert np.all(a[n if given and capn else 0:] == SENT), what       # behind min(count, capacity) nothing is touched; NULL: nothing is
    if D:
        got = D.read()
        exp = D.with_rows(want.D)
        assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
    P.unchanged()
    if N:
        fams = sort_families(b) + ["gf2_lf2_pair_count_kernel", "gf2_lf2_scan_group_kernelIx"]
        if capn:
            fams.append("gf2_lf2_pair_scatter_kernelILi%dE" % dev.lf2_plan(N, ncols, b)[6])
        assert_route(k0, census(L), fams)
    return count, want


def run_sort(dev, L, words, ncols, c0, b, skeys=True, layout=EE, stream=None):
    """gf2_class_sort_dev alone against the numpy stable sort"""
    import torch
    N = words.shape[0]
    order, sk = lf.class_sort(words, c0, b)
    P = View(dev, N, ncols, layout, 17 * N + c0, words)
    to, po = guarded(max(N, 1))
    tk, pk = guarded(max(N, 1))
    torch.cuda.synchronize()
    k0 = census(L)
    assert dev.class_sort(P.m, c0, b, order=po, skeys=pk if skeys else dev.SKIP, stream=stream) == (None, None)
    torch.cuda.synchronize()
    got, gk = read_guarded(to), read_guarded(tk)
    what = (N, ncols, c0, b, layout)
    assert np.array_equal(np.sort(got[:N]), np.arange(N)), what                      # a permutation
    assert np.array_equal(got[:N], order), (what, np.flatnonzero(got[:N] != order)[:8])
    assert np.all(got[N:] == SENT) and np.all(gk[N if skeys else 0:] == SENT), what
    if skeys:
        assert np.array_equal(gk[:N], sk) and np.all(np.diff(gk[:N]) >= 0), what
        ties = np.diff(gk[:N]) == 0
        assert np.all(np.diff(got[:N])[ties] > 0), what                              # ties in ascending row order
    P.unchanged()
    if N:
        assert_route(k0, census(L), sort_families(b))
    return order, sk


# ---- pass boundaries and window positions ----------------------------------------------------------------------------------------

WINDOWS = [(256, c0, b) for b in (0, 1, 7, 8, 9, 16, 17, 24, 25, 30) for c0 in (0, 37)]
WINDOWS += [(256, 50, 30),                                       # across a word boundary
            (256, 256 - 30, 30), (256, 256 - 9, 9),             # c0 + b == ncols, a multiple of 64
            (200, 200 - 17, 17), (130, 130 - 9, 9),             # ... and not one (130: the window crosses into the short word)
            (130, 64, 8), (200, 128, 25)]                        # from bit 0 of the second / third word


@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: "%d-c%d-b%d" % c)
def test_windows(dev, L, case):
    ncols, c0, b = case
    N = 300 if b < 8 else 2 * T + 5           # few classes: few rows, or the pairs are too many
    k = drawn(N, b, N // 3, 100 + c0 + b)
    if b >= 8:
        k[::7] ^= 1 << (b - 1)                # the highest bit of the key, which only the last pass sees
    words = keyed(N, ncols, c0, b, k, 200 + c0 + b)
    run_sort(dev, L, words, ncols, c0, b, layout=OO if c0 else EE)
    count, want = run(dev, L, words, ncols, c0, b, layouts=(OO, EE) if c0 else (EE, OE))
    assert count > N // 2 and (b == 0 or not lf.keys(want.D, c0, b).any())      # the window of D is zero


# ---- row counts --------------------------------------------------------------------------------------------------------------------

def count_cases():
    around = lambda name, n: [(name + "-1", n - 1), (name, n), (name + "+1", n + 1), ("2%s+5" % name, 2 * n + 5), ("3%s+1" % name, 3 * n + 1)]  # noqa: E731
    return [(str(n), n) for n in (0, 1, 2, 63, 64, 65)] + around("T", T) + around("R", R)


@pytest.mark.parametrize("case", count_cases(), ids=lambda c: c[0])
def test_row_counts(dev, L, case):
    N = case[1]
    ncols, c0, b = 128, 60, 9               # two passes; the window crosses a word boundary
    words = keyed(N, ncols, c0, b, drawn(N, b, max(N // 3, 1), 900 + N), 901 + N)
    order, _ = run_sort(dev, L, words, ncols, c0, b, layout=OE)
    assert len(order) == N
    count, _ = run(dev, L, words, ncols, c0, b, layouts=(OE, EE))
    if N < 2:
        assert count == 0
    run(dev, L, words, ncols, c0, b, cap="equal", layouts=(EE, OO), lo=False)


# ---- key distributions -------------------------------------------------------------------------------------------------------------

def test_one_class(dev, L):
    """all keys equal; 2R + 100 rows: the class of the third run began two runs earlier"""
    N, ncols, c0, b = 2 * R + 100, 64, 20, 12
    words = keyed(N, ncols, c0, b, np.full(N, 0xABC), 1)
    order, sk = run_sort(dev, L, words, ncols, c0, b)
    assert np.array_equal(order, np.arange(N))
    count, want = run(dev, L, words, ncols, c0, b, layouts=(EO, EE))
    assert count == N * (N - 1) // 2 and want.hi[-1] == N - 1 and want.lo[-1] == N - 2
    run(dev, L, words[:700], ncols, c0, 0)               # b == 0: one class whatever the bits say


def test_all_keys_distinct(dev, L):
    N, ncols, c0, b = 2 * T + 5, 256, 37, 14
    rng = np.random.default_rng(2)
    words = keyed(N, ncols, c0, b, rng.permutation(1 << b)[:N], 2)
    run_sort(dev, L, words, ncols, c0, b)
    assert run(dev, L, words, ncols, c0, b, cap=7)[0] == 0       # nothing is written
    assert run(dev, L, words, ncols, c0, b, cap="zero")[0] == 0
    # descending keys: the sort reverses the pool
    words = keyed(N, ncols, c0, b, np.arange(N)[::-1], 3)
    order, _ = run_sort(dev, L, words, ncols, c0, b, layout=OO)
    assert np.array_equal(order, np.arange(N)[::-1])
    # ... in classes of three: every class keeps its rows in ascending order
    words = keyed(N, ncols, c0, b, (N - 1 - np.arange(N)) // 3, 4)
    order, _ = run_sort(dev, L, words, ncols, c0, b)
    assert list(order[:6]) == [N - 3, N - 2, N - 1, N - 6, N - 5, N - 4]
    assert run(dev, L, words, ncols, c0, b)[0] >= N - 3


def test_two_alternating_values(dev, L):
    """stability: two classes that interleave over every tile, wave and round"""
    ncols, c0, b = 128, 5, 17
    N = 2 * T + 5
    k = np.where(np.arange(N) & 1, 3 << 9, 5 << 9)          # they differ in the second digit alone
    order, _ = run_sort(dev, L, keyed(N, ncols, c0, b, k, 5), ncols, c0, b)
    assert np.array_equal(order[:(N - 1) // 2], np.arange(1, N, 2)) and np.array_equal(order[(N - 1) // 2:], np.arange(0, N, 2))
    N = 701
    count, _ = run(dev, L, keyed(N, ncols, c0, b, k[:N], 6), ncols, c0, b)
    assert count == 350 * 349 // 2 + 351 * 350 // 2


@pytest.mark.parametrize("b", [8, 12])
def test_random_keys_three_rows_per_class(dev, L, b):
    N, ncols, c0 = 3 << b, 256, 101
    words = g.random_words(N, ncols, b)
    run_sort(dev, L, words, ncols, c0, b)
    count, _ = run(dev, L, words, ncols, c0, b)
    assert abs(count - 1.5 * N) <= 10 * np.sqrt(N)       # three standard deviations (tests/test_lf2_reference.py)


def test_one_class_holds_half_the_rows(dev, L):
    N, ncols, c0, b = 3000, 130, 64, 12
    rng = np.random.default_rng(7)
    k = rng.integers(0, 1 << b, N)
    k[rng.permutation(N)[:N // 2]] = 0x5A5                  # scattered over the pool
    words = keyed(N, ncols, c0, b, k, 7)
    run_sort(dev, L, words, ncols, c0, b)
    count, _ = run(dev, L, words, ncols, c0, b, layouts=(OO, OO))
    assert count >= (N // 2) * (N // 2 - 1) // 2


def test_a_class_starts_at_a_run_boundary(dev, L):
    """R rows of distinct keys, then classes whose first sorted position is R, and one that ends with position 2R - 1"""
    ncols, c0, b = 128, 33, 16
    k = np.concatenate([np.arange(R), np.full(50, R + 5), np.arange(R - 50 - 9) + 2 * R, np.full(9, 5 * R), np.full(4, 6 * R)])
    rng = np.random.default_rng(8)
    k = k[rng.permutation(len(k))]
    words = keyed(len(k), ncols, c0, b, k, 8)
    order, sk = run_sort(dev, L, words, ncols, c0, b)
    assert sk[R - 1] != sk[R] == sk[R + 49] and sk[2 * R - 10] != sk[2 * R - 9] == sk[2 * R - 1] != sk[2 * R]
    count, _ = run(dev, L, words, ncols, c0, b)
    assert count == 50 * 49 // 2 + 36 + 6


@pytest.mark.parametrize("where", ["highest", "lowest"])
def test_keys_that_differ_in_one_digit(dev, L, where):
    ncols, c0 = 200, 90
    N = T + 500
    for b in (24, 30):
        top = b - 8 * (dev.lf2_plan(N, ncols, b)[0] - 1)           # the bits of the last pass
        rng = np.random.default_rng(b)
        k = rng.integers(0, 1 << top, N) << (b - top) if where == "highest" else rng.integers(0, 256, N)
        k = k | (0 if where == "highest" else 0x2B << 8)          # the other digits are equal (and not zero)
        words = keyed(N, ncols, c0, b, k, b)
        run_sort(dev, L, words, ncols, c0, b, layout=EO)
        run(dev, L, words, ncols, c0, b, cap=3000)


# ---- row widths and alignment ------------------------------------------------------------------------------------------------------

WIDTHS = [1, 64, 65, 130, 200, 256, 257, 320, 513, 1030, 4100]


def test_the_widths_cover_the_lanes(dev):
    lanes = {dev.lf2_plan(100, n, 4)[6] for n in WIDTHS}
    assert lanes == {dev.lf2_plan(100, n, 4)[6] for n in range(1, 8200, 61)} == {1, 2, 8, 64}
    assert any(n % 64 for n in WIDTHS) and any(n % 64 == 0 for n in WIDTHS) and any(g.width(n) % 2 for n in WIDTHS)


@pytest.mark.parametrize("layouts", LAYOUT_PAIRS, ids=lambda p: "P%d%d-D%d%d" % (p[0] + p[1]))
@pytest.mark.parametrize("ncols", WIDTHS)
def test_widths_and_alignment(dev, L, ncols, layouts):
    b = min(5, ncols)
    c0 = ncols - b               # the window ends with the row
    N = 400 if ncols < 5 else R + 77    # two runs
    words = keyed(N, ncols, c0, b, drawn(N, b, 20, ncols), ncols)
    words[N - 3] = words[2]      # a repeated row: a zero row in D
    count, want = run(dev, L, words, ncols, c0, b, cap="more", layouts=layouts)
    assert not want.D[list(zip(want.lo, want.hi)).index((2, N - 3))].any()
    run(dev, L, words, ncols, c0, b, cap="less", layouts=layouts, hi=False)


# ---- capacity ----------------------------------------------------------------------------------------------------------------------

def capacity_pool():
    N, ncols, c0, b = 2500, 257, 250, 7
    return g.random_words(N, ncols, 55), ncols, c0, b


@pytest.mark.parametrize("given", ["lo+hi", "lo", "hi", "neither"])
@pytest.mark.parametrize("cap", ["zero", 1, "count-1", "equal", "more", "in a position", "in a class"])
def test_capacity(dev, L, cap, given):
    words, ncols, c0, b = capacity_pool()
    k = lf.keys(words, c0, b)
    count = lf.pair_count(k)
    sizes = np.unique(k, return_counts=True)[1]
    n0 = int(sizes[0])
    assert n0 >= 5 and count > 20000
    capn = {"count-1": count - 1,
            "in a position": n0 * (n0 - 1) // 2 + 3 + 2,           # inside the outputs of the fourth member of the second class
            "in a class": n0 * (n0 - 1) // 2 + 6}.get(cap, cap)    # behind the fourth member of the second class
    got, want = run(dev, L, words, ncols, c0, b, cap=capn, lo="lo" in given, hi="hi" in given, layouts=(OO, OE))
    assert got == count
    if cap == "in a position":
        assert want.hi[-1] == want.hi[-2] != want.hi[-3] and len(set(lf.keys(words[want.hi[-3:]], c0, b))) == 1


def test_a_count_past_2_to_31(dev, L):
    """70 000 rows of one key: 2 449 965 000 pairs.  1000 of them are written; the count-only form says the same"""
    N, ncols, c0, b = 70000, 96, 70, 21
    words = keyed(N, ncols, c0, b, np.full(N, 0x12345), 70)
    count, want = run(dev, L, words, ncols, c0, b, cap=1000, layouts=(EE, OO))
    assert count == 2449965000 > 1 << 31 and len(want.lo) == 1000
    assert run(dev, L, words, ncols, c0, b, cap="zero")[0] == count


# ---- the wrappers, composition -----------------------------------------------------------------------------------------------------

def test_wrappers_size_their_results(dev):
    N, ncols, c0, b = 5000, 100, 41, 10
    words = g.random_words(N, ncols, 8)
    want = lf.lf2(words, ncols, c0, b)
    P = dev.DMat.from_words(words, ncols)
    D, count, lo, hi = dev.lf2_reduce(P, c0, b)          # cap=None: a count-only call first
    assert D.nrows == want.count == len(want.lo) and np.array_equal(D.to_words(), want.D)
    assert int(count.read(None)[0]) == D.nrows and count.read(None).dtype == np.int64
    assert np.array_equal(lo.read(None), want.lo) and np.array_equal(hi.read(None), want.hi)
    D = P.lf2_reduce(c0, b)
    assert D.nrows == want.count and np.array_equal(D.to_words(), want.D)
    order, skeys = dev.class_sort(P, c0, b)
    ro, rk = lf.class_sort(words, c0, b)
    assert np.array_equal(order.read(None), ro) and np.array_equal(skeys.read(None), rk)
    order, skeys = dev.class_sort(P, c0, b, skeys=dev.SKIP)
    assert skeys is None and np.array_equal(order.read(None), ro)
    # no pair: an empty matrix; no row: empty arrays
    E = dev.DMat.from_words(words[:1], ncols).lf2_reduce(c0, b)
    assert E.nrows == 0 and E.ncols == ncols
    order, skeys = dev.class_sort(dev.DMat.wrap(None, 0, ncols, 2), c0, b)
    assert len(order.read(None)) == 0 and len(skeys.read(None)) == 0
    assert np.array_equal(P.to_words(), words)


def test_lo_and_hi_feed_the_gathers(dev):
    """D == gather(P, hi) ^ gather(P, lo): the index outputs go to the gathers as the device arrays they are"""
    N, ncols, c0, b = 9000, 300, 100, 11
    words = g.random_words(N, ncols, 17)
    want = lf.lf2(words, ncols, c0, b)
    P = dev.DMat.from_words(words, ncols)
    D, count, lo, hi = dev.lf2_reduce(P, c0, b, cap=want.count)
    D2 = dev.DMat(want.count, ncols)
    dev.gather_rows(P, hi.ptr, D=D2)
    dev.gather_rows(P, lo.ptr, D=D2, accumulate=True)
    assert np.array_equal(D2.to_words(), want.D) and np.array_equal(D.to_words(), want.D)


def test_two_calls_give_the_same_bits(dev, L):
    N, ncols, c0, b = 3 * T + 1, 192, 77, 12
    words = g.random_words(N, ncols, 21)
    P = dev.DMat.from_words(words, ncols)
    results = []
    for _ in range(2):
        D, count, lo, hi = dev.lf2_reduce(P, c0, b, cap=2 * N)
        order, skeys = dev.class_sort(P, c0, b)
        n = int(count.read(None)[0])
        results.append((n, D.to_words()[:n], lo.read(None)[:n], hi.read(None)[:n], order.read(None), skeys.read(None)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert results[0][0] == lf.pair_count(lf.keys(words, c0, b))


# ---- dirty scratch, streams, past 4 GiB --------------------------------------------------------------------------------------------

def test_on_dirty_scratch(dev, L):
    """pair buffers, digit counts, sorted order and run sums come from a cache in which every block holds a pattern, and no block
    comes fresh from the driver"""
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for N, ncols, b in ((3 * R + 5, 128, 9), (2 * T + 77, 320, 25)):
            words = keyed(N, ncols, 33, b, drawn(N, b, N // 3, N), N)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arenas are new
            h0 = cache.hits()
            run(dev, L, words, ncols, 33, b, stream=stream)
            run_sort(dev, L, words, ncols, 33, b, stream=stream)
            assert cache.hits() - h0 >= 2
            cache.no_fresh("the LF2 round on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pool is written by gf2_dmat_fill_random on the caller's stream, behind a sleep; the same round is enqueued twice behind it,
    into two destinations, before anything synchronises.  Both must hold what the yardstick makes of the seeded pool."""
    import torch
    N, ncols, c0, b, seed = 20011, 200, 57, 13, 0xB1C
    words = lr.seeded_words(seed, ncols, np.arange(N))
    want = lf.lf2(words, ncols, c0, b)
    count = want.count
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    tp = torch.full((N, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    P = dev.DMat.from_torch(tp, ncols)
    outs = []
    for _ in range(2):
        td = torch.full((count + 2, 4), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.from_torch(td, ncols), guarded(2), guarded(count + 2), guarded(count + 2), guarded(N)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    P.fill_random(seed, s)
    for td, D, (tc, pc), (tl, pl), (th, ph), (to, po) in outs:
        dev.lf2_reduce(P, c0, b, D=D, count=pc, lo=pl, hi=ph, stream=s)
        dev.class_sort(P, c0, b, order=po, skeys=dev.SKIP, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for td, D, (tc, pc), (tl, pl), (th, ph), (to, po) in outs:
        rows = td.cpu().numpy().view(np.uint64)
        assert count_of(tc) == count
        assert np.array_equal(rows[:count], want.D) and np.all(rows[count:] == np.uint64(0x1111111111111111))
        assert np.array_equal(read_guarded(tl)[:count], want.lo) and np.array_equal(read_guarded(th)[:count], want.hi)
        assert np.array_equal(read_guarded(to), lf.class_sort(words, c0, b)[0])


def test_a_view_of_a_parent_past_4gib(dev, L):
    """70 000 rows of 128 columns, 8192 words apart: the last rows start behind byte offset 2^32 of the parent.  Only the view's words
    are written (gf2_copy_block_dev from a compact upload); D is compact"""
    import torch
    N, ncols, ld, c0, b = 70000, 128, 8192, 60, 15
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((N, ld), dtype=torch.int64, device="cuda")
    assert N * ld * 8 > lr.LIMIT_BYTES
    words = g.random_words(N, ncols, 70)
    r_hi = lr.straddle(ld, N)[1]
    words[N - 1] = words[5]                       # a pair on either side of 2^32: a zero row
    P = dev.DMat.wrap(t.data_ptr() + 8 * 6, N, ncols, ld, keep=t)
    dev.copy_block(P, 0, 0, dev.DMat.from_words(words, ncols), 0, 0, N, ncols)
    want = lf.lf2(words, ncols, c0, b)
    D, count, lo, hi = dev.lf2_reduce(P, c0, b, cap=want.count + 1)
    assert int(count.read(None)[0]) == want.count
    assert np.array_equal(lo.read(None)[:-1], want.lo) and np.array_equal(hi.read(None)[:-1], want.hi)
    assert np.array_equal(D.to_words()[:-1], want.D)
    assert (want.hi > r_hi).sum() > 0 and not want.D[list(zip(want.lo, want.hi)).index((5, N - 1))].any()
    order, skeys = dev.class_sort(P, c0, b)
    assert np.array_equal(order.read(None), lf.class_sort(words, c0, b)[0])
    del t, P, D
    gc.collect()
    torch.cuda.empty_cache()


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def lpn_samples(seed, k, N=3072, tau=1 / 8):
    rng = np.random.default_rng(seed)
    secret = rng.integers(0, 2, k, dtype=np.uint8)
    samples = rng.integers(0, 2, (N, k), dtype=np.uint8)
    errors = (rng.random(N) < tau).astype(np.uint8)
    label = (samples.astype(np.int64) @ secret.astype(np.int64) + errors) % 2
    bits = np.concatenate([samples, label[:, None].astype(np.uint8)], axis=1)
    return g.bits_to_words(bits), secret


def errors_of(words, ncols, k):
    """the errors of all 2^k secrets over the first k columns against the last column, in numpy"""
    bits = g.words_to_bits(words, ncols).astype(np.int64)
    s = (np.arange(1 << k)[:, None] >> np.arange(k)[None, :]) & 1
    return bits, ((bits[:, :k] @ s.T) % 2 != bits[:, ncols - 1:ncols]).sum(axis=0)


@pytest.mark.parametrize("seed", [0, 3])
def test_lf2_end_to_end(dev, seed):
    """12 secret columns, 10 window columns, the label; N = 3072 = 3 * 2^10, noise 1/8: one LF2 round, the errors of the 2^12 secrets
    that are left, the minimum -- one chain, one synchronisation at its end"""
    import torch
    words, secret = lpn_samples(seed, 22)
    r = lf.lf2(words, 23, 12, 10)
    bits, errors = errors_of(r.D, 23, 12)
    assert abs(r.count - 4606) <= 10 * np.sqrt(3072) and not bits[:, 12:22].any()     # N (N - 1) / 2^11, three standard deviations
    low = int(sum(int(x) << j for j, x in enumerate(secret[:12])))
    ranked = np.argsort(errors, kind="stable")
    assert ranked[0] == low and errors[ranked[0]] <= 1200 and errors[ranked[1]] >= 1900      # the yardstick alone finds the secret
    P = dev.DMat.from_words(words, 23)
    cap = 1.6 * 3072
    te, pe = guarded(1 << 12)
    tm, pm = guarded(2)
    torch.cuda.synchronize()
    D, count, _, _ = dev.lf2_reduce(P, 12, 10, cap=r.count, lo=dev.SKIP, hi=dev.SKIP)
    dev.lpn_errors(D, 0, 12, 22, out=pe)
    dev.min_weight(pe, 1 << 12, idx=pm, val=pm + 4)
    torch.cuda.synchronize()
    assert int(count.read(None)[0]) == r.count <= cap
    assert np.array_equal(D.to_words(), r.D)
    assert np.array_equal(read_guarded(te), errors)
    assert list(read_guarded(tm)) == [low, int(errors[low])]
    Q = P.lf2_reduce(12, 10)
    assert Q.nrows == r.count and np.array_equal(Q.lpn_errors(0, 12, 22), errors)


@pytest.mark.parametrize("seed", [0, 4])
def test_lf1_then_lf2_end_to_end(dev, seed):
    """four more secret columns, taken by an LF1 round in front of the LF2 round.  The 16 representatives of that round carry their
    noise into every row of their class, so the margin of the true secret varies with the seed: these two leave 870 errors and more"""
    import torch
    words, secret = lpn_samples(seed, 26)
    r1 = l1.lf1(words, 27, 22, 4)
    r2 = lf.lf2(r1.D, 27, 12, 10)
    bits, errors = errors_of(r2.D, 27, 12)
    assert r1.D.shape[0] == 3072 - 16 and not bits[:, 12:26].any()
    low = int(sum(int(x) << j for j, x in enumerate(secret[:12])))
    ranked = np.argsort(errors, kind="stable")
    assert ranked[0] == low and errors[ranked[1]] - errors[ranked[0]] >= 300      # the yardstick alone finds the secret
    P = dev.DMat.from_words(words, 27)
    te, pe = guarded(1 << 12)
    tm, pm = guarded(2)
    torch.cuda.synchronize()
    D1, _, _, _ = dev.lf1_reduce(P, 22, 4, cap=3056, src=dev.SKIP)
    D2, count, _, _ = dev.lf2_reduce(D1, 12, 10, cap=r2.count, lo=dev.SKIP, hi=dev.SKIP)
    dev.lpn_errors(D2, 0, 12, 26, out=pe)
    dev.min_weight(pe, 1 << 12, idx=pm, val=pm + 4)
    torch.cuda.synchronize()
    assert int(count.read(None)[0]) == r2.count
    assert np.array_equal(D2.to_words(), r2.D)
    assert np.array_equal(read_guarded(te), errors)
    assert list(read_guarded(tm)) == [low, int(errors[low])]
