"""GPU tests of include/m4ri_hip_unique.h: gf2_sort_rows_dev and gf2_unique_rows_dev bit for bit against the numpy yardstick of
tests/unique_ref.py (itself checked against big integers by tests/test_unique_reference.py): `order`, `head`, `keep` up to
min(count, cap), `count` and `rep`, all of them exactly.

The harness is that of tests/test_gpu_near.py: P is a window of a dirty parent (View of tests/test_gpu_lf1.py: the excess bits of the
last word are dirty too) and the parent is compared afterwards; the int outputs lie between sentinels and hold a pattern before the
call; which kernels ran, and how many launches a call took, is read from the launch census and compared with gf2_sort_rows_plan.

The pools (pool_bits): rows drawn from a dictionary of about nrows / 3 values of the range, so classes have several members scattered
through the pool; random junk in every bit outside the range; for every column of the range a planted pair of rows that differs in
that column alone -- whatever the cut into windows is, a bit that is dropped or counted twice changes the result --; and a pair that
differs only in the columns c0 - 1 and c1, which must come out equal.

The sort tile (4096 rows) and the run of the head kernels are read from gf2_lf2_plan / gf2_sort_rows_plan.  Every kernel of
gf2_unique.hip is launched by every call of run() with rows and a non-empty range."""
import gc

import numpy as np
import pytest

import dev_views as dv
import dirty_pool as dp
import gf2util as g
import limits_ref as lr
import unique_ref as ur
from census_util import assert_route, census
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded

pytestmark = pytest.mark.gpu

BIG = 3 * 4096 + 5
OWN = ["gf2_unique_rekey_kernel", "gf2_unique_heads_kernel", "gf2_unique_carry_kernel", "gf2_unique_fill_kernel", "gf2_unique_rep_kernel"]


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

def pool_bits(n, ncols, c0, c1, seed):
    """-> (n, ncols) uint8 as the module docstring says"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, ncols), dtype=np.uint8)                   # junk in every column
    w = c1 - c0
    if n and w:
        values = rng.integers(0, 2, (max(n // 3, 1), w), dtype=np.uint8)
        bits[:, c0:c1] = values[rng.integers(0, len(values), n)]
    perm = rng.permutation(n)
    for t in range(min(w, max(n // 2 - 2, 0))):                             # column c0 + t: rows a and b differ there alone
        a, b = perm[2 * t], perm[2 * t + 1]
        bits[b, c0:c1] = bits[a, c0:c1]
        bits[b, c0 + t] ^= 1
    if n >= 4:                                                              # equal on the range, different right outside it
        a, b = perm[-1], perm[-2]
        bits[b, c0:c1] = bits[a, c0:c1]
        if c0 > 0:
            bits[b, c0 - 1] = bits[a, c0 - 1] ^ 1
        if c1 < ncols:
            bits[b, c1] = bits[a, c1] ^ 1
    return bits


def pool(n, ncols, c0, c1, seed):
    return g.bits_to_words(pool_bits(n, ncols, c0, c1, seed)) if ncols else np.zeros((n, 0), dtype=np.uint64)


def with_values(n, ncols, c0, c1, seed, ids, id_bits=16):
    """rows whose range holds: `ids[i]` in its id_bits most significant columns, below them random bits that are a function of the id
    (equal ids: equal values; the order of the values is the order of the ids); junk outside the range"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, ncols), dtype=np.uint8)
    low = rng.integers(0, 2, (int(max(ids)) + 1, c1 - c0 - id_bits), dtype=np.uint8)
    bits[:, c0:c1 - id_bits] = low[ids]
    bits[:, c1 - id_bits:c1] = (np.asarray(ids)[:, None] >> np.arange(id_bits)) & 1
    return g.bits_to_words(bits)


def capacity(cap, count):
    return {"zero": 0, "less": count // 2, "equal": count, "more": count + 7}[cap] if isinstance(cap, str) else cap


def launches(before, after, family=""):
    return sum(v - before.get(k, 0) for k, v in after.items() if family in k)


def run(dev, L, words, ncols, c0, c1, layout=EE, cap="more", head=True, rep=True, stream=None, want=None, P=None):
    """gf2_sort_rows_dev and gf2_unique_rows_dev on a dirty window against the yardstick -> the yardstick's result"""
    import torch
    n = len(words)
    if want is None:
        want = ur.everything(words, c0, c1)
    capn = capacity(cap, want.count)
    m = min(capn, want.count)
    if P is None:
        P = View(dev, n, ncols, layout, 5 * n + c0, words)
    (to, po), (th, ph), (tk, pk), (tc, pc), (tr, pr) = guarded(n), guarded(n), guarded(capn), guarded(1), guarded(n)
    torch.cuda.synchronize()
    k0 = census(L)
    assert dev.sort_rows(P.m, c0, c1, order=po, head=ph if head else dev.SKIP, stream=stream) == (None, None)
    k1 = census(L)
    out = dev.unique_rows(P.m, c0, c1, keep=pk if capn else dev.SKIP, cap=capn, count=pc, rep=pr if rep else dev.SKIP, stream=stream)
    assert out == (None, None, None)
    torch.cuda.synchronize()
    k2 = census(L)
    what = (n, ncols, c0, c1, layout, cap, head, rep)
    order, heads, keep, count, reps = (read_guarded(t) for t in (to, th, tk, tc, tr))
    if n:
        assert np.array_equal(order, want.order), (what, np.flatnonzero(order != want.order)[:8])
        assert int(count[0]) == want.count, (what, count[0], want.count)
    else:
        assert int(count[0]) == 0, what                                     # *count = 0 and nothing else is written
    assert np.array_equal(heads, want.head if head else np.full(n, SENT)), (what, np.flatnonzero(heads != want.head)[:8])
    assert np.array_equal(reps, want.rep if rep else np.full(n, SENT)), (what, np.flatnonzero(reps != want.rep)[:8])
    assert np.array_equal(keep[:m], want.keep[:m]) and np.all(keep[m:] == SENT), what   # behind min(count, cap) nothing is touched
    P.unchanged()
    plan = dev.sort_rows_plan(n, ncols, c0, c1)
    if n == 0:
        assert launches(k0, k2) == 0, what
        return want
    assert launches(k0, k1) == plan[4] + (3 if head else 0), (what, launches(k0, k1), plan)
    assert launches(k1, k2) == plan[5] - (0 if capn else 1), (what, launches(k1, k2), plan)
    assert launches(k0, k1, "gf2_unique_") == plan[1] + (3 if head else 0) and launches(k1, k2, "gf2_unique_") == plan[1] + 4, what
    if c1 > c0:
        assert_route(k0, k1, ["gf2_unique_rekey_kernel", "gf2_lf2_sort_count_kernel", "gf2_lf2_sort_scatter_kernel"])
        assert launches(k0, k2, "gf2_lf2_iota") == 0 and launches(k0, k2, "gf2_lf2_sort_scatter") == 2 * plan[0], what
    else:
        assert launches(k0, k2, "gf2_lf2_iota") == 2 and launches(k0, k2, "gf2_lf2_sort") == 0, what
    if head:
        assert_route(k0, k1, OWN[1:4])
    assert_route(k1, k2, OWN[1:] + ["gf2_weight_select_count_kernel", "gf2_weight_select_scan_kernel"])
    assert launches(k1, k2, "gf2_weight_select_scatter") == (1 if capn else 0), what
    return want


# ---- row counts --------------------------------------------------------------------------------------------------------------------

def test_the_sizes_are_the_plans(dev):
    assert dev.lf2_plan(1000, 200, 24)[4] == 4096 and dev.sort_rows_plan(1000, 200, 57, 200)[8] == 1024


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, BIG])
def test_row_counts(dev, L, n):
    ncols, c0, c1 = 200, 57, 200
    words = pool(n, ncols, c0, c1, 100 + n)
    want = run(dev, L, words, ncols, c0, c1, layout=[EE, EO, OE, OO][n % 4])
    if n >= 300:
        assert n // 4 < want.count < n and want.count == len(want.keep)     # classes of several members, and the planted singletons


# ---- ranges ------------------------------------------------------------------------------------------------------------------------

RANGES = [(1, 0, 1), (64, 0, 64), (200, 57, 57), (200, 57, 87), (200, 57, 88), (130, 1, 129), (256, 0, 256), (257, 0, 257), (257, 63, 257),
          (1000, 3, 997)]


@pytest.mark.parametrize("case", RANGES, ids=lambda c: "%d-c%d-%d" % c)
def test_ranges(dev, L, case):
    """one window and several, windows that cross word boundaries, a last window of 1 .. 24 bits, the empty range; 5000 rows: two sort
    tiles and five runs, and room for a planted pair per column of the widest range"""
    ncols, c0, c1 = case
    n = 5000
    bits = pool_bits(n, ncols, c0, c1, 7 * ncols + c0)
    words = g.bits_to_words(bits)
    want = run(dev, L, words, ncols, c0, c1, layout=[EE, EO, OE, OO][RANGES.index(case) % 4])
    if c0 == c1:
        assert want.count == 1 and not want.head.any() and not want.rep.any() and np.array_equal(want.order, np.arange(n))
        return
    # what the pool promises, read off the yardstick: a row and its representative agree on the range, and some do although both
    # neighbouring columns differ
    assert np.array_equal(bits[want.rep, c0:c1], bits[:, c0:c1]) and 1 < want.count < n
    if c0 > 0 and c1 < ncols:
        assert ((bits[want.rep, c0 - 1] != bits[:, c0 - 1]) & (bits[want.rep, c1] != bits[:, c1])).any()


@pytest.mark.parametrize("case", [c for c in RANGES if c[2] - c[1] <= 30], ids=lambda c: "%d-c%d-%d" % c)
def test_order_equals_the_class_sort_on_the_device(dev, case):
    ncols, c0, c1 = case
    for n in (1, 4097, BIG):
        P = dev.DMat.from_words(pool(n, ncols, c0, c1, n + c1), ncols)
        order, head = dev.sort_rows(P, c0, c1)
        corder, skeys = dev.class_sort(P, c0, c1 - c0)
        a, b = order.read(None), corder.read(None)
        assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (case, n)
        k = skeys.read(None)                                                   # the heads are where the sorted keys change
        assert np.array_equal(head.read(None), np.maximum.accumulate(np.where(np.r_[True, k[1:] != k[:-1]], np.arange(n), 0)))


# ---- class shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["all-equal", "all-distinct", "giant-then-distinct", "pairs-across-borders"])
def test_class_shapes(dev, L, shape):
    n, ncols, c0, c1 = BIG, 200, 57, 200
    rng = np.random.default_rng(len(shape))
    if shape == "all-equal":
        sorted_ids = np.zeros(n, dtype=np.int64)
    elif shape == "all-distinct":
        sorted_ids = np.arange(n)
    elif shape == "giant-then-distinct":
        sorted_ids = np.maximum(np.arange(n) - 9000, 0)                         # 9001 rows of the lowest value: it spans eight runs
    else:
        s = np.arange(n)
        sorted_ids = s - (s >= 1024) - (s >= 4096)                              # positions 1023 | 1024 and 4095 | 4096 hold one value each
    ids = sorted_ids[rng.permutation(n)]                                        # scattered through the pool
    words = with_values(n, ncols, c0, c1, 31 + len(shape), ids)
    want = run(dev, L, words, ncols, c0, c1, layout=OO)
    assert np.array_equal(ids[want.order], sorted_ids)
    if shape == "all-equal":
        assert want.count == 1 and not want.head.any() and not want.rep.any() and want.keep.tolist() == [0]   # the carry crosses every run
        assert np.array_equal(want.order, np.arange(n))
    elif shape == "all-distinct":
        assert want.count == n and np.array_equal(want.keep, np.arange(n)) and np.array_equal(want.head, np.arange(n))
    elif shape == "giant-then-distinct":
        assert want.count == n - 9000 and not want.head[:9001].any() and np.array_equal(want.head[9001:], np.arange(9001, n))
    else:
        assert want.count == n - 2 and (want.head[1024], want.head[4096]) == (1023, 4095)
        assert np.array_equal(np.flatnonzero(want.head != np.arange(n)), [1024, 4096])


# ---- capacity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", ["zero", 1, "count-1", "equal", "more"])
def test_capacity(dev, L, cap):
    """cap == 0 with keep NULL, a capacity below, equal to and above the count; rep and head NULL and given"""
    n, ncols, c0, c1 = 3000, 130, 1, 129
    words = pool(n, ncols, c0, c1, 55)
    want = ur.everything(words, c0, c1)
    assert 1000 < want.count < n
    capn = want.count - 1 if cap == "count-1" else cap
    for head, rep in ((True, True), (False, False), (True, False), (False, True)):
        run(dev, L, words, ncols, c0, c1, cap=capn, head=head, rep=rep, layout=EO, want=want)


# ---- the kept rows -----------------------------------------------------------------------------------------------------------------

def test_gather_of_the_kept_rows_and_the_wrappers(dev):
    import torch
    n, ncols, c0, c1 = 6000, 300, 40, 260
    words = pool(n, ncols, c0, c1, 8)
    want = ur.everything(words, c0, c1)
    P = dev.DMat.from_words(words, ncols)
    keep, count, rep = dev.unique_rows(P, c0, c1)                                # neither keep nor cap: a count-only call first
    assert keep.count == want.count == int(count.read(None)[0]) and np.array_equal(keep.read(None), want.keep)
    assert np.array_equal(rep.read(None), want.rep)
    D, bad = dev.gather_rows(P, keep.ptr, D=dev.DMat(want.count, ncols), bad=None)
    assert bad is False and np.array_equal(D.to_words(), words[want.keep])
    U = P.unique_rows(c0, c1)
    assert (U.nrows, U.ncols) == (want.count, ncols) and np.array_equal(U.to_words(), words[want.keep])
    order = P.sort_rows(c0, c1)
    assert np.array_equal(order.read(None), want.order)
    order, head = dev.sort_rows(P, c0, c1)
    assert np.array_equal(order.read(None), want.order) and np.array_equal(head.read(None), want.head)
    assert dev.sort_rows(P, c0, c1, head=dev.SKIP)[1] is None
    # the whole row is the default range
    whole = ur.everything(words, 0, ncols)
    assert np.array_equal(P.sort_rows().read(None), whole.order) and P.unique_rows().nrows == whole.count
    # keep preset to -1: the rows behind *count gather as zero
    t = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    keep, count, rep = dev.unique_rows(P, c0, c1, keep=t.data_ptr(), cap=n, rep=dev.SKIP)
    assert keep is None and rep is None and int(count.read(None)[0]) == want.count
    D, bad = dev.gather_rows(P, t.data_ptr(), D=dev.DMat(n, ncols), bad=None)
    got = D.to_words()
    assert bad is False and np.array_equal(got[:want.count], words[want.keep]) and not got[want.count:].any()
    keep, count, rep = dev.unique_rows(P, c0, c1, keep=dev.SKIP)                 # the count alone
    assert keep is None and int(count.read(None)[0]) == want.count
    with pytest.raises(ValueError):
        dev.unique_rows(P, c0, c1, keep=t.data_ptr())
    with pytest.raises(ValueError):
        dev.unique_rows(P, c0, c1, count=t.data_ptr())
    with pytest.raises(Exception, match="columns"):
        dev.sort_rows(P, 5, 4)
    E = dev.DMat(0, ncols).unique_rows()
    assert (E.nrows, E.ncols) == (0, ncols)
    # two lists are equal as sets iff their kept rows, sorted, are equal as matrices
    other = dev.DMat.from_words(words[np.random.default_rng(1).permutation(n)], ncols)
    def canonical(M):
        kept = M.unique_rows()
        return dev.gather_rows(kept, kept.sort_rows().ptr, D=dev.DMat(kept.nrows, ncols))[0].to_words()

    assert np.array_equal(canonical(P), canonical(other)) and len(canonical(P)) == whole.count
    assert np.array_equal(P.to_words(), words)


def test_two_calls_give_the_same_bits(dev):
    n, ncols = 20000, 256
    P = dev.DMat.from_words(pool(n, ncols, 0, ncols, 3), ncols)
    results = []
    for _ in range(2):
        order, head = dev.sort_rows(P)
        keep, count, rep = dev.unique_rows(P, cap=n)
        results.append((order.read(None), head.read(None), keep.read(None)[:int(count.read(None)[0])], count.read(None), rep.read(None)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert 0 < int(results[0][3][0]) < n


# ---- views, dirty scratch, streams -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", dv.LAYOUTS)
def test_strided_offset_views_of_dirty_parents(dev, layout):
    """tests/dev_views.py: at least one dirty row above and two below the window, dirty words left and right of it; 8-byte-aligned
    rows, an odd ld, a base on an odd word; WIDE: a column range of a wider matrix.  Nothing of the parent is written"""
    n, ncols, c0, c1 = 4500, 300, 61, 290
    bits = pool_bits(n, ncols, c0, c1, 40 + dv.LAYOUTS.index(layout))
    P = dv.View(dev, n, ncols, layout, 41, g.bits_to_words(bits))
    want = ur.everything(P.window(), c0, c1)
    order, head = dev.sort_rows(P.m, c0, c1)
    keep, count, rep = dev.unique_rows(P.m, c0, c1, cap=n)
    assert np.array_equal(order.read(None), want.order) and np.array_equal(head.read(None), want.head)
    assert int(count.read(None)[0]) == want.count and np.array_equal(keep.read(None)[:want.count], want.keep)
    assert np.array_equal(rep.read(None), want.rep)
    P.unchanged("P")


def test_on_dirty_scratch(dev, L):
    """pairs, counts, carries, order, heads, flags and block counts come from a cache in which every block holds a pattern, and no
    block comes fresh from the driver"""
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for n, ncols, c0, c1 in ((BIG, 200, 57, 200), (9000, 257, 63, 257), (5000, 64, 0, 64)):
            words = pool(n, ncols, c0, c1, n)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run(dev, L, words, ncols, c0, c1, stream=stream, layout=OE)
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the row sort on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pool is gathered from a dictionary that gf2_dmat_fill_random writes on the caller's stream, behind a sleep; the same calls
    are enqueued twice behind it, into two sets of arrays, before anything synchronises.  Both must hold what the yardstick makes of
    the seeded dictionary."""
    import torch
    n, ncols, seed, c0, c1 = 9001, 200, 0x51DE, 10, 190
    dictionary = lr.seeded_words(seed, ncols, np.arange(n // 3))
    idx = np.random.default_rng(5).integers(0, n // 3, n).astype(np.int32)
    want = ur.everything(dictionary[idx], c0, c1)
    assert n // 4 < want.count <= n // 3
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    td = torch.full((n // 3, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    tp = torch.full((n, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    ti = torch.from_numpy(idx).cuda()
    S, P = dev.DMat.from_torch(td, ncols), dev.DMat.from_torch(tp, ncols)
    outs = [[guarded(n), guarded(n), guarded(n), guarded(1), guarded(n)] for _ in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    S.fill_random(seed, s)
    dev.gather_rows(S, ti.data_ptr(), D=P, stream=s)
    for (to, po), (th, ph), (tk, pk), (tc, pc), (tr, pr) in outs:
        dev.sort_rows(P, c0, c1, order=po, head=ph, stream=s)
        dev.unique_rows(P, c0, c1, keep=pk, cap=n, count=pc, rep=pr, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for (to, po), (th, ph), (tk, pk), (tc, pc), (tr, pr) in outs:
        assert np.array_equal(read_guarded(to), want.order) and np.array_equal(read_guarded(th), want.head)
        keep = read_guarded(tk)
        assert int(read_guarded(tc)[0]) == want.count and np.array_equal(keep[:want.count], want.keep) and np.all(keep[want.count:] == SENT)
        assert np.array_equal(read_guarded(tr), want.rep)


# ---- past 4 GiB ----------------------------------------------------------------------------------------------------------------------

def test_a_view_of_a_parent_past_4gib(dev, L):
    """600 rows of 200 columns, 2^20 words apart: the rows from 512 on start behind byte offset 2^32 of the parent.  Only the view's
    words are written (gf2_copy_block_dev from a compact upload)"""
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
    words = pool(n, ncols, c0, c1, 90)
    hi = np.arange(n) >= 512                                      # the rows behind 2^32
    words[599] = words[3]                                          # classes with a member on either side
    words[7] = words[550]
    want = ur.everything(words, c0, c1)
    assert want.rep[599] == want.rep[3] < 512 and want.rep[550] == want.rep[7] < 512 and hi[want.keep].sum() > 10
    P = dev.DMat.wrap(t.data_ptr() + 8 * 6, n, ncols, ld, keep=t)
    dev.copy_block(P, 0, 0, dev.DMat.from_words(words, ncols), 0, 0, n, ncols)
    order, head = dev.sort_rows(P, c0, c1)
    keep, count, rep = dev.unique_rows(P, c0, c1, cap=n)
    assert np.array_equal(order.read(None), want.order) and np.array_equal(head.read(None), want.head)
    assert int(count.read(None)[0]) == want.count and np.array_equal(keep.read(None)[:want.count], want.keep)
    assert np.array_equal(rep.read(None), want.rep)
    del t, P
    gc.collect()
    torch.cuda.empty_cache()


# ---- census ------------------------------------------------------------------------------------------------------------------------

def test_every_kernel_of_the_module_is_launched(dev, L):
    """each kernel of gf2_unique.hip by name, before and after one call of each entry"""
    words = pool(2500, 130, 1, 129, 4)
    P = dev.DMat.from_words(words, 130)
    k0 = census(L)
    dev.sort_rows(P, 1, 129)
    dev.unique_rows(P, 1, 129, cap=2500)
    k1 = census(L)
    for name in OWN:
        assert launches(k0, k1, name) >= 1, name
    assert launches(k0, k1, "gf2_unique_") == launches(k0, k1, "gf2_unique_rekey") + 3 + 3 + 1
