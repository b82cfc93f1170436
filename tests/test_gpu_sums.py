"""GPU tests of include/m4ri_hip_sums.h: gf2_subset_sums_dev and gf2_unrank_subsets_dev bit for bit against the numpy yardstick of
tests/sums_ref.py (itself checked against the definition by tests/test_sums_reference.py): the rows of D, the words around D, idx
and wt and the ints around them.

Every operand is a window of a dirty parent (View of tests/test_gpu_lf1.py): random bits in every word of the parent -- the rows
before and behind the window, the words left and right of it, the excess bits of the last word of S and base -- and the whole parent
of D is compared afterwards.  The int outputs lie between sentinels and hold a pattern before the call.

R (ranks per workgroup), the lanes per row and the kernel (S in LDS or from global memory) are read from gf2_subset_sums_plan, never
written down here; which kernel ran is read from the launch census.  The case lists are module constants, and a test that needs no
device checks that they reach every kernel id the plan can return."""
import gc
import itertools

import numpy as np
import pytest

import gf2util as g
import limits_ref as lr
import sums_ref as sr
from census_util import assert_route, census
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded

gpu = pytest.mark.gpu
OUTPUTS = ("rows", "idx", "wt")
LAYOUT_TRIPLES = [(EE, EE, EE), (EO, OE, OO), (OO, EE, EO), (OE, OO, EE), (EE, EO, OE)]   # (S, base, D): every parity on every side


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


def plan(n, ncols, p, count):
    """(kernel id, threads, R, lanes, LDS bytes, workgroups, scratch bytes) of gf2_subset_sums_plan"""
    from m4ri_rust_amd import device
    return device.subset_sums_plan(n, ncols, p, count)


def plan_r():
    try:
        return plan(200, 70, 2, 5000)[2]
    except Exception:   # not built yet: the fixture builds; test_the_cases_are_the_plans checks the size
        return 1024


R = plan_r()            # ranks per workgroup of a list as short as the ones below


def kernel_of(n, ncols, p, count):
    kid, _, _, lanes, lds, _, _ = plan(n, ncols, p, count)
    assert (kid >= 4) == (lds == 0) and lanes == (1, 2, 8, 64)[kid & 3]
    return "gf2_subset_sums_kernelILi%dELb%dEE" % (lanes, 0 if kid >= 4 else 1)


def largest_staged(ncols):
    """the largest n whose rows the plan still copies into LDS (a bisection of the plan's answers)"""
    lo, hi = 2, 1 << 20
    assert plan(lo, ncols, 2, 1)[0] < 4 <= plan(hi, ncols, 2, 1)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(mid, ncols, 2, 1)[0] < 4 else (lo, mid)
    return lo


def run(dev, L, S, ncols, p, base=None, rank0=0, count=None, given=OUTPUTS, wcols=None, layouts=(EE, EE, EE), stream=None, views=None):
    """one gf2_subset_sums_dev call on dirty windows against the yardstick -> (the yardstick's outputs, the views of S and base).
    S, base: packed words; views: the views of an earlier call on the same S and base"""
    import torch
    n = S.shape[0]
    wc0, wc1 = (0, ncols) if wcols is None else wcols
    want = sr.sums(S, ncols, p, base, rank0, count, wc0, wc1)
    count = len(want.idx)
    if views is None:
        views = (View(dev, n, ncols, layouts[0], 11 * n + p, S), View(dev, 1, ncols, layouts[1], 7 * n + p, base) if base is not None else None)
    VS, VB = views
    D = View(dev, count, ncols, layouts[2], 13 * n + rank0 % 1000) if "rows" in given else None
    ti, pi = guarded(max(count * p, 1))
    tw, pw = guarded(max(count, 1))
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.subset_sums(VS.m, p, base=VB.m if VB else None, rank0=rank0, count=None if D else count, D=D.m if D else None,
                          idx=pi if "idx" in given else dev.SKIP, wt=pw if "wt" in given else dev.SKIP, wcols=(wc0, wc1), store=D is not None,
                          stream=stream)
    assert out == (D.m if D else None, None, None)
    torch.cuda.synchronize()
    what = (n, ncols, p, base is not None, rank0, count, given, (wc0, wc1), layouts)
    got_i, got_w = read_guarded(ti), read_guarded(tw)
    if "idx" in given:
        assert np.array_equal(got_i[:count * p].reshape(count, p), want.idx), (what, np.argwhere(got_i[:count * p].reshape(count, p) != want.idx)[:8])
    assert np.all(got_i[count * p if "idx" in given else 0:] == SENT), what       # behind the window nothing is touched; NULL: nothing is
    if "wt" in given:
        assert np.array_equal(got_w[:count], want.wt), (what, np.flatnonzero(got_w[:count] != want.wt)[:8])
    assert np.all(got_w[count if "wt" in given else 0:] == SENT), what
    if D:
        got, exp = D.read(), D.with_rows(want.D)
        assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
    VS.unchanged()
    if VB:
        VB.unchanged()
    if count:
        assert_route(k0, census(L), [kernel_of(n, ncols, p, count)])
    return want, views


def words(n, ncols, seed):
    return g.random_words(n, ncols, seed)


# ---- the case lists ------------------------------------------------------------------------------------------------------------------

SMALL = [(p, n) for p in (1, 2, 3, 4) for n in (p, p + 1, 9)]                      # 70 columns
CARRY = [(2, 200, 100), (3, 40, 20), (4, 24, 12)]                                   # (p, n, c): a block of the top level starts at C(c, p)
CARRY_COUNTS = [("1", 1), ("63", 63), ("64", 64), ("65", 65), ("R-1", R - 1), ("R", R), ("R+1", R + 1), ("2R+5", 2 * R + 5)]
WIDTHS = [1, 64, 65, 130, 200, 256, 257, 320, 513, 1030, 4100]
WIDTH_SHAPE = (3, 20)                                                                # p, n: 1140 sums, two workgroups
PATH_WIDTHS = [64, 256, 320, 4100]                                                   # one width per lane count: S just inside LDS, and just outside
WEIGHT_RANGES = [(0, 0), (77, 77), (0, 200), (70, 100), (60, 140), (3, 193), (129, 200), (191, 200)]


def path_cases():
    """(n, ncols, p, rank0, count): the largest n that the plan stages in LDS and the next one; the window ends with the list and
    begins 300 ranks before the last block of the top level, or R + 400 ranks before the end where that is longer"""
    out = []
    for ncols in PATH_WIDTHS:
        n = largest_staged(ncols)
        for m in (n, n + 1):
            count = max(R + 400, m + 299)
            out.append((m, ncols, 2, sr.count(m, 2) - count, count))
    return out


def shapes_of_the_cases():
    """(n, ncols, p, count) of every call of the lists above"""
    shapes = [(n, 70, p, sr.count(n, p)) for p, n in SMALL]
    shapes += [(n, 130, p, c) for p, n, _ in CARRY for _, c in CARRY_COUNTS]
    shapes += [(WIDTH_SHAPE[1], ncols, WIDTH_SHAPE[0], sr.count(WIDTH_SHAPE[1], WIDTH_SHAPE[0])) for ncols in WIDTHS]
    shapes += [(n, ncols, p, count) for n, ncols, p, _, count in path_cases()]
    return shapes


def test_the_cases_are_the_plans(built):
    """needs no device: R is the plan's, the case lists reach every kernel id that the plan can return, and every lane count on either
    path; the widths include every alignment case"""
    assert R == plan_r() == plan(24, 130, 4, 2 * R + 5)[2] == plan(200, 130, 2, 1)[2] and R >= 256
    ids = {plan(*s)[0] for s in shapes_of_the_cases()}
    possible = {plan(n, ncols, p, 1)[0] for ncols in range(1, 9000, 37) for n in (4, 100, 3000, 70000) for p in (1, 4)}
    assert ids == possible == set(range(8)), (sorted(ids), sorted(possible))
    assert {plan(20, n, 3, 1140)[3] for n in WIDTHS} == {1, 2, 8, 64} and plan(20, 200, 3, 1140)[5] == 2
    assert any(n % 64 for n in WIDTHS) and any(n % 64 == 0 for n in WIDTHS) and any(g.width(n) % 2 for n in WIDTHS)
    for n, ncols, p, rank0, count in path_cases():
        assert 0 <= rank0 and rank0 + count <= sr.count(n, p) and count > R
    staged = [plan(n, ncols, p, count)[0] < 4 for n, ncols, p, _, count in path_cases()]
    assert staged == [True, False] * len(PATH_WIDTHS)
    assert plan(200, 70, 2, 100)[6] == 0                    # no scratch: there is no dirty-scratch case to run


# ---- small and exhaustive ------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("p,n", SMALL)
def test_small_lists_from_every_rank(dev, L, p, n):
    ncols = 70
    S, base = words(n, ncols, 10 * n + p), words(1, ncols, 99)
    total = sr.count(n, p)
    views = None
    for rank0 in range(total):                                 # the window to the end
        _, views = run(dev, L, S, ncols, p, base, rank0=rank0, layouts=(OE, EO, OO), wcols=(3, 69), views=views)
    run(dev, L, S, ncols, p, base, rank0=0, count=1, views=views)
    run(dev, L, S, ncols, p, None, rank0=total - 1, count=1, layouts=(EE, EE, OE))
    run(dev, L, S, ncols, p, None, rank0=total, count=0)       # nothing is written


# ---- run and carry boundaries --------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("shape", CARRY, ids=lambda s: "p%d-n%d" % s[:2])
@pytest.mark.parametrize("case", CARRY_COUNTS, ids=lambda c: c[0])
def test_counts_and_block_boundaries(dev, L, shape, case):
    p, n, c = shape
    count = case[1]
    ncols = 130
    assert plan(n, ncols, p, count)[2] == R
    S, base = words(n, ncols, 5 * n), words(1, ncols, 6 * n)
    block = sr.count(c, p)                                     # the first rank whose c_p is c
    assert [int(x) for x in sr.subsets(n, p, block - 1, 2)[:, -1]] == [c - 1, c] and block + 2 * R + 5 <= sr.count(n, p)
    views = None
    for rank0 in (0, block, block - 1, block - 37):            # the last: the boundary lies inside the first wave's stride
        _, views = run(dev, L, S, ncols, p, base, rank0=rank0, count=count, layouts=(EE, OO, EO), wcols=(60, 129), views=views)


# ---- row widths and alignment --------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("layouts", LAYOUT_TRIPLES, ids=lambda t: "S%d%d-b%d%d-D%d%d" % (t[0] + t[1] + t[2]))
@pytest.mark.parametrize("ncols", WIDTHS)
def test_widths_and_alignment(dev, L, ncols, layouts):
    p, n = WIDTH_SHAPE
    S, base = words(n, ncols, ncols), words(1, ncols, ncols + 1)
    S[7] = S[3] ^ S[11] ^ base[0]                             # a zero row in D
    lo = min(3, ncols - 1)
    want, views = run(dev, L, S, ncols, p, base, layouts=layouts, wcols=(lo, ncols))
    t = sr.rank((3, 7, 11))
    assert not want.D[t].any() and want.wt[t] == 0 and tuple(want.idx[t]) == (3, 7, 11)
    run(dev, L, S, ncols, p, None, rank0=500, count=333, layouts=layouts, given=("rows", "wt"), wcols=(0, ncols - lo))


# ---- both paths of S -----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("at", range(2 * len(PATH_WIDTHS)), ids=lambda i: "%d-%s" % (PATH_WIDTHS[i // 2], ("lds", "global")[i % 2]))
def test_s_in_lds_and_from_global_memory(dev, L, at):
    n, ncols, p, rank0, count = path_cases()[at]
    S, base = words(n, ncols, 3 * ncols + at), words(1, ncols, 5 * ncols + at)
    want, _ = run(dev, L, S, ncols, p, base, rank0=rank0, count=count, layouts=(EO, EE, OE) if at % 2 else (EE, OE, EE), wcols=(0, min(ncols, 50)))
    assert want.idx[:, 1].max() == n - 1 and want.idx[:, 0].min() == 0 and len({int(x) for x in want.idx[:, 1]}) >= 2     # the last rows of S, a carry


# ---- outputs -------------------------------------------------------------------------------------------------------------------------

SUBSETS = [tuple(s) for r in (1, 2, 3) for s in itertools.combinations(OUTPUTS, r)]


@gpu
@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("given", SUBSETS, ids=lambda s: "+".join(s))
def test_every_legal_subset_of_the_outputs(dev, L, given, with_base):
    """rows not stored included: idx alone, wt alone, both"""
    ncols, n = 257, 30
    S, base = words(n, ncols, 41), words(1, ncols, 42)
    for p, rank0, count in ((2, 7, 400), (4, 100, R + 50), (1, 0, 30)):
        run(dev, L, S, ncols, p, base if with_base else None, rank0=rank0, count=count, given=given, layouts=(OO, EO, OE), wcols=(10, 250))


@gpu
def test_rows_not_stored_need_an_array(dev):
    S = dev.DMat.from_words(words(10, 100, 1), 100)
    with pytest.raises(dev._lib.HipError, match="idx or wt"):
        dev.subset_sums(S, 2, store=False, idx=dev.SKIP, wt=dev.SKIP)


@gpu
@pytest.mark.parametrize("wcols", WEIGHT_RANGES, ids=lambda w: "%d-%d" % w)
def test_weight_ranges(dev, L, wcols):
    """empty, the whole row, inside one word, across three words, ending at ncols with ncols % 64 != 0; with the rows and without"""
    ncols, n, p = 200, 25, 3
    S, base = words(n, ncols, 77), words(1, ncols, 78)
    want, views = run(dev, L, S, ncols, p, base, wcols=wcols, layouts=(EO, OE, EE))
    bits = g.words_to_bits(want.D, ncols)
    assert len(want.wt) == 2300 and np.array_equal(want.wt, bits[:, wcols[0]:wcols[1]].sum(axis=1))
    if wcols[1] > wcols[0] + 20:
        assert want.wt.max() > want.wt.min()
    run(dev, L, S, ncols, p, base, wcols=wcols, given=("wt",), views=views)


# ---- large ranks, D past 4 GiB -------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("where", ["2^31", "2^32", "end"])
def test_large_ranks(dev, L, where):
    """131072 rows of 64 columns, p = 2: C(n, 2) = 8 589 869 056 passes 2^33; windows of 3000 rows across 2^31, across 2^32, at the end"""
    n, ncols = 131072, 64
    total = sr.count(n, 2)
    rank0 = {"2^31": (1 << 31) - 1500, "2^32": (1 << 32) - 1500, "end": total - 3000}[where]
    S, base = words(n, ncols, 131), words(1, ncols, 132)
    want, _ = run(dev, L, S, ncols, 2, base, rank0=rank0, count=3000, layouts=(EE, EE, EO))
    assert sr.rank(tuple(int(x) for x in want.idx[0])) == rank0 and sr.rank(tuple(int(x) for x in want.idx[-1])) == rank0 + 2999
    if where == "end":
        assert tuple(want.idx[-1]) == (n - 2, n - 1)


@gpu
def test_d_is_a_view_at_the_end_of_a_parent_past_4gib(dev, L):
    """the parent: 70 000 rows, 8192 words apart; D: its last 3000 rows from word 6 on, every one of them behind byte offset 2^32"""
    import torch
    rows, ld, count, ncols, n, p = 70000, 8192, 3000, 200, 30, 3
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((rows, ld), dtype=torch.int64, device="cuda")
    r0 = rows - count
    assert 8 * r0 * ld > lr.LIMIT_BYTES
    t[r0 - 1:, :16] = 0x1111111111111111                     # the words around the view
    S, base = words(n, ncols, 70), words(1, ncols, 71)
    want = sr.sums(S, ncols, p, base, 1000, count, 64, 200)
    D = dev.DMat.wrap(t.data_ptr() + 8 * (r0 * ld + 6), count, ncols, ld, keep=t)
    ti, pi = guarded(count * p)
    tw, pw = guarded(count)
    dev.subset_sums(dev.DMat.from_words(S, ncols), p, base=dev.DMat.from_words(base, ncols), rank0=1000, D=D, idx=pi, wt=pw, wcols=(64, 200))
    torch.cuda.synchronize()
    around = t[r0 - 1:, :16].cpu().numpy().view(np.uint64)
    exp = np.full((count + 1, 16), 0x1111111111111111, dtype=np.uint64)
    exp[1:, 6:6 + g.width(ncols)] = want.D
    assert np.array_equal(around, exp), np.argwhere(around != exp)[:8]
    assert np.array_equal(read_guarded(ti).reshape(count, p), want.idx) and np.array_equal(read_guarded(tw), want.wt)
    del t, D
    gc.collect()
    torch.cuda.empty_cache()


# ---- determinism, streams ------------------------------------------------------------------------------------------------------------

@gpu
def test_two_calls_give_the_same_bits(dev, L):
    n, ncols, p = 60, 192, 3
    S, base = dev.DMat.from_words(words(n, ncols, 21), ncols), dev.DMat.from_words(words(1, ncols, 22), ncols)
    results = []
    for _ in range(2):
        D, idx, wt = dev.subset_sums(S, p, base=base, rank0=11, count=3 * R + 1)
        results.append((D.to_words(), idx.read(None), wt.read(None)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    want = sr.sums(words(n, ncols, 21), ncols, p, words(1, ncols, 22), 11, 3 * R + 1)
    assert np.array_equal(results[0][0], want.D) and np.array_equal(results[0][1], want.idx) and np.array_equal(results[0][2], want.wt)


@gpu
def test_behind_pending_work_on_a_caller_stream(dev, L):
    """S and base are written by gf2_dmat_fill_random on the caller's stream, behind a sleep; the same call is enqueued twice behind
    it, into two destinations, before anything synchronises.  Both must hold what the yardstick makes of the seeded rows."""
    import torch
    n, ncols, p, seed, rank0, count = 300, 200, 2, 0xB1C, 5000, 9001
    S, base = lr.seeded_words(seed, ncols, np.arange(n)), lr.seeded_words(seed + 1, ncols, np.arange(1))
    want = sr.sums(S, ncols, p, base, rank0, count, 0, 57)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ts = torch.full((n, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    tb = torch.full((1, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    A, B = dev.DMat.from_torch(ts, ncols), dev.DMat.from_torch(tb, ncols)
    outs = []
    for _ in range(2):
        td = torch.full((count + 2, 4), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.wrap(td.data_ptr(), count, ncols, 4, keep=td), guarded(count * p), guarded(count)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    A.fill_random(seed, s)
    B.fill_random(seed + 1, s)
    for td, D, (ti, pi), (tw, pw) in outs:
        dev.subset_sums(A, p, base=B, rank0=rank0, D=D, idx=pi, wt=pw, wcols=(0, 57), stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for td, D, (ti, pi), (tw, pw) in outs:
        rows = td.cpu().numpy().view(np.uint64)
        assert np.array_equal(rows[:count], want.D) and np.all(rows[count:] == np.uint64(0x1111111111111111))
        assert np.array_equal(read_guarded(ti).reshape(count, p), want.idx) and np.array_equal(read_guarded(tw), want.wt)


# ---- gf2_unrank_subsets_dev ----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_unrank_random_ranks(dev, L, p):
    import torch
    n = {1: 100000, 2: 131072, 3: 3000, 4: 400}[p]
    total = sr.count(n, p)
    rng = np.random.default_rng(p)
    count = 1000
    for rank0 in (0, total // 3):
        span = min(total - rank0, (1 << 31) - 1)
        rel = rng.integers(0, span, count)
        rel[:4] = (0, span - 1, span // 2, 1)
        rel[10:20] = -1                                          # what a caller finds behind the count of a selection
        want = np.array([sr.unrank(rank0 + int(r), p) if r >= 0 else (-1,) * p for r in rel], dtype=np.int32)
        tr = torch.from_numpy(rel.astype(np.int32)).cuda()
        ti, pi = guarded(count * p)
        tb, pb = guarded(1)
        k0 = census(L)
        out = dev.unrank_subsets(tr.data_ptr(), count, p, n, rank0=rank0, idx=pi, bad=pb)
        assert out == (None, None)
        torch.cuda.synchronize()
        assert_route(k0, census(L), ["gf2_unrank_subsets_kernel"])
        assert np.array_equal(read_guarded(ti).reshape(count, p), want), (p, rank0)
        assert int(read_guarded(tb)[0]) == SENT                  # no rank was bad: `bad` stays as it was
        assert np.array_equal(tr.cpu().numpy(), rel.astype(np.int32))


@gpu
def test_unrank_reports_ranks_outside_the_list(dev, L):
    import torch
    p, n = 3, 50
    total = sr.count(n, p)
    for rank0, rel in ((0, [5, total, 7, -2, total - 1, -1, (1 << 31) - 1]), (total - 10, [9, 10, 0, -(total - 10) - 1, -(total - 10)])):
        good = [0 <= rank0 + r < total and r != -1 for r in rel]
        want = np.array([sr.unrank(rank0 + r, p) if ok else (-1,) * p for r, ok in zip(rel, good)], dtype=np.int32)
        tr = torch.tensor(rel, dtype=torch.int32, device="cuda")
        ti, pi = guarded(len(rel) * p)
        tb = torch.zeros(1, dtype=torch.int32, device="cuda")
        dev.unrank_subsets(tr.data_ptr(), len(rel), p, n, rank0=rank0, idx=pi, bad=tb.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(read_guarded(ti).reshape(len(rel), p), want) and int(tb[0]) == 1
    # the wrapper's own arrays: a list of ranks goes up, idx and bad come back
    idx, bad = dev.unrank_subsets([0, 1, total - 1, -1], 4, p, n)
    assert bad is False and [tuple(r) for r in idx.read(None)] == [(0, 1, 2), (0, 1, 3), (47, 48, 49), (-1, -1, -1)]
    assert dev.unrank_subsets([0, total], 2, p, n)[1] is True
    assert dev.unrank_subsets([3], 1, 3, 2, bad=dev.SKIP)[0].read(None).tolist() == [[-1, -1, -1]]      # n < p: no subset at all
    assert dev.unrank_subsets([], 0, p, n)[0] is None


# ---- the wrappers, composition -------------------------------------------------------------------------------------------------------

@gpu
def test_wrappers_size_their_results(dev):
    n, ncols, p = 40, 100, 3
    S, base = words(n, ncols, 8), words(1, ncols, 9)
    want = sr.sums(S, ncols, p, base, 0, None, 20, 90)
    A, B = dev.DMat.from_words(S, ncols), dev.DMat.from_words(base, ncols)
    D, idx, wt = dev.subset_sums(A, p, base=B, wcols=(20, 90))               # count=None: all of them
    assert D.nrows == dev.subset_count(n, p) == 9880 and np.array_equal(D.to_words(), want.D)
    assert idx.read(None).shape == (9880, 3) and np.array_equal(idx.read(None), want.idx) and np.array_equal(wt.read(None), want.wt)
    assert np.array_equal(A.subset_sums(p, base=B).to_words(), want.D)
    assert np.array_equal(A.subset_sums(1).to_words(), S) and A.subset_sums(1).nrows == n
    D, idx, wt = dev.subset_sums(A, p, base=B, rank0=9000, idx=dev.SKIP)      # from a rank to the end
    assert D.nrows == 880 and idx is None and np.array_equal(D.to_words(), want.D[9000:])
    assert np.array_equal(wt.read(None), sr.sums(S, ncols, p, base, 9000).wt)
    D, idx, wt = dev.subset_sums(A, p, rank0=17, count=100, store=False, wt=dev.SKIP)
    assert D is None and wt is None and np.array_equal(idx.read(None), want.idx[17:117])
    E = dev.DMat.from_words(S[:2], ncols).subset_sums(3)                      # n < p: the empty list
    assert E.nrows == 0 and E.ncols == ncols
    with pytest.raises(ValueError, match="do not fit a matrix"):
        dev.subset_sums(dev.DMat.wrap(A.s.data, 131072, 64, 1), 2)
    with pytest.raises(ValueError, match="passes 2\\^62"):
        dev.subset_sums(dev.DMat.wrap(A.s.data, 200000, 64, 1), 4)
    assert np.array_equal(A.to_words(), S) and np.array_equal(B.to_words(), base)


@gpu
def test_idx_feeds_the_row_gather(dev):
    """D == base ^ gather(S, c_1) ^ ... ^ gather(S, c_p): idx goes to gf2_gather_rows_dev as the device array it is.  p = 1: one
    accumulating gather onto copies of base.  p = 3: one gather of count * p rows, G[t * p + i] = S[c_i], then G seen as count rows
    of p blocks side by side, the blocks XORed into the copies of base"""
    n, ncols = 50, 300
    S, base = words(n, ncols, 17), words(1, ncols, 18)
    A = dev.DMat.from_words(S, ncols)
    for p, rank0, count in ((1, 3, 40), (3, 1234, 5000)):
        want = sr.sums(S, ncols, p, base, rank0, count)
        D, idx, wt = dev.subset_sums(A, p, base=dev.DMat.from_words(base, ncols), rank0=rank0, count=count, wt=dev.SKIP)
        D2 = dev.DMat.from_words(np.tile(base, (count, 1)), ncols)
        if p == 1:
            dev.gather_rows(A, idx.ptr, D=D2, accumulate=True)
        else:
            G = dev.DMat(count * p, ncols)
            dev.gather_rows(A, idx.ptr, D=G)
            for i in range(p):
                block = dev.DMat.wrap(G.s.data + 8 * i * G.ld, count, ncols, p * G.ld, keep=G)
                dev.copy_block(D2, 0, 0, block, 0, 0, count, ncols, accumulate=True)
        assert wt is None and np.array_equal(D2.to_words(), want.D) and np.array_equal(D.to_words(), want.D)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def stern_instance(seed):
    """Q: 128 x 80 random bits.  The error has two columns in each half of Q (i1 < i2 in the left 40, j1 < j2 in the right 40) and 5
    more ones among the rows 8 .. 127 (e1); s = Q[:, i1] ^ Q[:, i2] ^ Q[:, 40 + j1] ^ Q[:, 40 + j2] ^ e1 -> (Q, s, (i1, i2), (j1, j2),
    e1), all as bits"""
    rng = np.random.default_rng(seed)
    Q = rng.integers(0, 2, (128, 80), dtype=np.uint8)
    i = tuple(sorted(int(x) for x in rng.choice(40, 2, replace=False)))
    j = tuple(sorted(int(x) for x in rng.choice(40, 2, replace=False)))
    e1 = np.zeros(128, dtype=np.uint8)
    e1[rng.choice(np.arange(8, 128), 5, replace=False)] = 1
    return Q, Q[:, i[0]] ^ Q[:, i[1]] ^ Q[:, 40 + j[0]] ^ Q[:, 40 + j[1]] ^ e1, i, j, e1


def stern_by_the_yardstick(seed):
    """the lists, their join on [0, 8) with the weights on [8, 128), and the assertion that the planted pair is the only light one"""
    import join_ref as jr
    Q, s, i, j, e1 = stern_instance(seed)
    left, right = g.bits_to_words(np.ascontiguousarray(Q[:, :40].T)), g.bits_to_words(np.ascontiguousarray(Q[:, 40:].T))
    sw = g.bits_to_words(s[None, :])
    L1, L2 = sr.sums(left, 128, 2, sw), sr.sums(right, 128, 2)
    assert len(L1.idx) == len(L2.idx) == 780
    J = jr.join(L1.D, L2.D, 128, 0, 8, 8, 128)
    light = np.flatnonzero(J.wt <= 5)
    assert 2000 <= J.count <= 2800 and len(light) == 1 and np.sort(J.wt)[1] >= 30          # the yardstick alone finds the pair, and only it
    t = int(light[0])
    assert tuple(L1.idx[J.ia[t]]) == i and tuple(L2.idx[J.ib[t]]) == j and np.array_equal(g.words_to_bits(J.D[t:t + 1], 128)[0], e1)
    return Q, sw, i, j, e1, L1, L2, J, t


@pytest.mark.parametrize("seed", range(6))
def test_the_stern_instances_have_one_light_pair(seed):
    """needs no device: what test_stern_with_two_columns_per_half relies on"""
    stern_by_the_yardstick(seed)


@gpu
@pytest.mark.parametrize("seed", range(6))
def test_stern_with_two_columns_per_half(dev, seed):
    """Stern with p = 2 per half: L1 = all XORs of two columns of the left half, each ^ s, L2 = those of the right half, both by
    gf2_subset_sums_dev; the join on the columns [0, 8) with the weights over [8, 128), the selection of the weights up to 5, the
    gather of the hit, ia and ib of the hit unranked to the columns -- one chain, one synchronisation at its end"""
    import torch
    Q, sw, i, j, e1, L1, L2, J, t = stern_by_the_yardstick(seed)
    Qt = dev.transpose(dev.DMat.from_words(g.bits_to_words(Q), 80))
    A, B = dev.submatrix(Qt, 0, 0, 40, 128), dev.submatrix(Qt, 40, 0, 80, 128)
    sd = dev.DMat.from_words(sw, 128)
    cap = 3000
    ints = lambda k, fill=0: torch.full((k,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
    ia, ib, wt, hits, nhits = ints(cap), ints(cap), ints(cap), ints(4, -1), ints(1)
    names = ints(8, 7)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    hit = dev.DMat(1, 128)
    torch.cuda.synchronize()
    D1 = dev.subset_sums(A, 2, base=sd, idx=dev.SKIP, wt=dev.SKIP)[0]
    D2 = dev.subset_sums(B, 2, idx=dev.SKIP, wt=dev.SKIP)[0]
    D = dev.join(D1, D2, 0, 8, cap=cap, count=count.data_ptr(), ia=ia.data_ptr(), ib=ib.data_ptr(), wt=wt.data_ptr(), wcols=(8, 128))[0]
    dev.select_weights(wt.data_ptr(), J.count, 0, 5, idx=hits.data_ptr(), cap=4, count=nhits.data_ptr())
    dev.gather_rows(D, hits.data_ptr(), D=hit)                      # the rows of the hits; -1: a zero row
    first = hits[:1].long()
    ranks = torch.cat([ia[first], ib[first]]).contiguous()          # ia[hit], ib[hit]: the ranks of the two halves of the hit
    dev.unrank_subsets(ranks.data_ptr(), 1, 2, 40, idx=names.data_ptr(), bad=dev.SKIP)
    dev.unrank_subsets(ranks.data_ptr() + 4, 1, 2, 40, idx=names.data_ptr() + 8, bad=dev.SKIP)
    torch.cuda.synchronize()
    assert D1.nrows == D2.nrows == 780 and int(count[0]) == J.count <= cap
    assert np.array_equal(D1.to_words(), L1.D) and np.array_equal(D2.to_words(), L2.D)
    assert np.array_equal(D.to_words()[:J.count], J.D) and np.array_equal(wt.cpu().numpy()[:J.count], J.wt)
    assert int(nhits[0]) == 1 and hits.cpu().tolist() == [t, -1, -1, -1]
    assert names.cpu().tolist() == [i[0], i[1], j[0], j[1], 7, 7, 7, 7]
    assert np.array_equal(g.words_to_bits(hit.to_words(), 128)[0], e1)


def lee_brickell_instance(seed):
    """S: 200 rows of 128 random bits; s = S[a] ^ S[b] ^ e with 5 ones in e -> (S, s, (a, b), e) as words, words, a tuple, bits"""
    rng = np.random.default_rng(100 + seed)
    S = rng.integers(0, 2, (200, 128), dtype=np.uint8)
    ab = tuple(sorted(int(x) for x in rng.choice(200, 2, replace=False)))
    e = np.zeros(128, dtype=np.uint8)
    e[rng.choice(128, 5, replace=False)] = 1
    return g.bits_to_words(S), g.bits_to_words((S[ab[0]] ^ S[ab[1]] ^ e)[None, :]), ab, e


def lee_brickell_by_the_yardstick(seed):
    S, sw, ab, e = lee_brickell_instance(seed)
    want = sr.sums(S, 128, 2, sw)
    light = np.flatnonzero(want.wt <= 5)
    assert len(want.wt) == 19900 and len(light) == 1 and np.sort(want.wt)[1] >= 30
    t = int(light[0])
    assert tuple(want.idx[t]) == ab and t == sr.rank(ab) and np.array_equal(g.words_to_bits(want.D[t:t + 1], 128)[0], e)
    return S, sw, ab, want, t


@pytest.mark.parametrize("seed", range(6))
def test_the_lee_brickell_instances_have_one_light_pair(seed):
    """needs no device: what test_lee_brickell_with_rows_not_stored relies on"""
    lee_brickell_by_the_yardstick(seed)


@gpu
@pytest.mark.parametrize("seed", range(6))
def test_lee_brickell_with_rows_not_stored(dev, seed):
    """Lee-Brickell with p = 2: the weights of s ^ S[a] ^ S[b] for all 19900 pairs, no row of them stored; the selection of the
    weights up to 5; the ranks of the hits unranked to the pairs -- one chain, one synchronisation at its end"""
    import torch
    S, sw, ab, want, t = lee_brickell_by_the_yardstick(seed)
    A, sd = dev.DMat.from_words(S, 128), dev.DMat.from_words(sw, 128)
    ints = lambda k, fill=0: torch.full((k,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
    wt, hits, nhits, names, bad = ints(19900), ints(4, -1), ints(1), ints(8, 7), ints(1)
    torch.cuda.synchronize()
    out = dev.subset_sums(A, 2, base=sd, store=False, idx=dev.SKIP, wt=wt.data_ptr())
    dev.select_weights(wt.data_ptr(), 19900, 0, 5, idx=hits.data_ptr(), cap=4, count=nhits.data_ptr())
    dev.unrank_subsets(hits.data_ptr(), 4, 2, 200, idx=names.data_ptr(), bad=bad.data_ptr())
    torch.cuda.synchronize()
    assert out == (None, None, None)
    assert np.array_equal(wt.cpu().numpy(), want.wt) and int(nhits[0]) == 1 and hits.cpu().tolist() == [t, -1, -1, -1]
    assert names.cpu().tolist() == [ab[0], ab[1], -1, -1, -1, -1, -1, -1] and int(bad[0]) == 0
