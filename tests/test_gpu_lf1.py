"""GPU tests of include/m4ri_hip_bkw.h: gf2_class_first_dev and gf2_lf1_reduce_dev bit for bit against the numpy LF1 round of
tests/lf1_ref.py (itself checked against the definition by tests/test_lf1_reference.py): the rows of D that are written, the rest of
D, the words around D, `count`, all of `first`, and `src` up to min(count, capacity).

Every operand of run() is a window of a dirty parent: random bits in every word of the parent -- the rows before and behind the window,
the words left and right of it, the excess bits of P's last word -- and the whole parent of D is compared afterwards, so a store outside
the rows that the contract names, or an excess bit that is not zero, fails the case.  `first`, `count` and `src` lie between sentinels
and hold a pattern before the call.

T (the largest b whose class firsts go through LDS), R (the rows a workgroup of the count / scatter kernels covers) and the lanes per
row are read from gf2_lf1_plan, never written down here; which kernels ran is read from the launch census."""
import gc
import os
import re

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import lf1_ref as lf
import limits_ref as lr
from census_util import assert_route, census

pytestmark = pytest.mark.gpu

SENT = 0x5EAD5EAD    # what an int output holds before the call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (ld odd, base on an odd word): 16-byte accesses are possible only with both even
EE, EO, OE, OO = (False, False), (False, True), (True, False), (True, True)
LAYOUT_PAIRS = [(EE, EE), (EE, OO), (OO, EE), (EO, OE), (OE, EO)]   # (P, D): every layout on either side, 16 bytes on both, one, none


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


def guarded(n):
    """n device ints between sentinels, all holding SENT; -> (tensor, address of the n ints)"""
    import torch
    t = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 16


def read_guarded(t):
    h = t.cpu().numpy()
    assert np.all(h[:4] == SENT) and np.all(h[-4:] == SENT), "a word next to an int output was written"
    return h[4:-4]


def T_of(dev):
    """the largest b of the LDS variant"""
    vs = [dev.lf1_plan(1000, 256, b)[0] for b in range(31)]
    return vs.index(1) - 1


def R_of(dev, ncols):
    return dev.lf1_plan(1000, ncols, 8)[3]


def scan_chunk():
    """block counts per round of the scan kernel (bkw_plan.h: kLf1ScanChunk = kLf1Threads * kLf1ScanItems)"""
    text = open(os.path.join(ROOT, "m4ri-rust_amd", "csrc", "bkw", "bkw_plan.h")).read()
    return int(re.search(r"kLf1Threads = (\d+);", text).group(1)) * int(re.search(r"kLf1ScanItems = (\d+);", text).group(1))


# ---- pools -----------------------------------------------------------------------------------------------------------------------

def set_keys(words, c0, b, k):
    """bits [c0, c0 + b) of row i <- k[i]"""
    if b == 0:
        return words
    k = np.asarray(k).astype(np.uint64)
    w0, s = c0 >> 6, c0 & 63
    lo = min(b, 64 - s)
    mask = np.uint64(((1 << lo) - 1) << s)
    words[:, w0] = (words[:, w0] & ~mask) | ((k << np.uint64(s)) & mask)
    if b > lo:
        mask = np.uint64((1 << (b - lo)) - 1)
        words[:, w0 + 1] = (words[:, w0 + 1] & ~mask) | ((k >> np.uint64(lo)) & mask)
    return words


def pool(N, ncols, c0, b, seed, classes=None):
    """N random rows; classes: the keys are drawn from that many random values below 2^b (None: as the random bits fall)"""
    words = g.random_words(N, ncols, seed)
    if classes is not None and b > 0 and N > 0:
        rng = np.random.default_rng(seed)
        values = rng.choice(1 << b, size=min(classes, 1 << b), replace=False) if b <= 20 else rng.integers(0, 1 << b, classes)
        set_keys(words, c0, b, values[rng.integers(0, len(values), N)])
    return words


class View:
    """nrows x ncols as a window of a parent that holds random bits in every word; `words` (clean) go into the window, the excess
    bits of the last word stay dirty"""

    def __init__(self, dev, nrows, ncols, layout, seed, words=None):
        import torch
        ld_odd, base_odd = layout
        w = g.width(ncols)
        ld = w + 3
        if bool(ld & 1) != ld_odd:
            ld += 1
        r0 = 1
        cw = 1 if bool((r0 * ld + 1) & 1) == base_odd else 2
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 1 << 64, (nrows + 3, ld), dtype=np.uint64)
        self.r0, self.cw, self.w, self.ncols = r0, cw, w, ncols
        if words is not None and nrows:
            dirty = self.host[r0:r0 + nrows, cw:cw + w].copy()
            self.host[r0:r0 + nrows, cw:cw + w] = words
            if ncols % 64:
                self.host[r0:r0 + nrows, cw + w - 1] |= dirty[:, -1] & ~np.uint64((1 << (ncols % 64)) - 1)
        self.t = torch.from_numpy(self.host.view(np.int64).copy()).cuda()
        assert self.t.data_ptr() % 16 == 0 and bool(ld & 1) == ld_odd and bool((r0 * ld + cw) & 1) == base_odd
        self.m = dev.DMat.wrap(self.t.data_ptr() + 8 * (r0 * ld + cw), nrows, ncols, ld, keep=self.t)

    def read(self):
        return self.t.cpu().numpy().view(np.uint64).reshape(self.host.shape)

    def unchanged(self):
        assert np.array_equal(self.read(), self.host), "the operand changed"

    def with_rows(self, rows):
        """the parent as it must look after the first len(rows) rows of the window were written as whole rows"""
        want = self.host.copy()
        want[self.r0:self.r0 + len(rows), self.cw:self.cw + self.w] = rows
        return want


def capacity(cap, count):
    return {"zero": 0, "less": count // 2, "equal": count, "more": count + 3}[cap] if isinstance(cap, str) else cap


def run(dev, L, words, ncols, c0, b, keep_zero=False, cap="more", src=True, layouts=(EE, EE), stream=None, want=None, route=True):
    """one gf2_lf1_reduce_dev call on dirty windows against the reference -> the reference's result"""
    import torch
    N = words.shape[0]
    want = lf.lf1(words, ncols, c0, b, keep_zero) if want is None else want
    count = len(want.src)
    capn = capacity(cap, count)
    P = View(dev, N, ncols, layouts[0], 11 * N + c0, words)
    D = View(dev, capn, ncols, layouts[1], 13 * N + b) if cap != "zero" else None
    Dm = D.m if D else dev.DMat.wrap(None, 0, ncols, g.width(ncols))
    tf, pf = guarded(1 << b)
    tc, pc = guarded(1)
    ts, ps = guarded(max(capn, 1))
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.lf1_reduce(P.m, c0, b, keep_zero=keep_zero, D=Dm, first=pf, count=pc, src=ps if src and capn else dev.SKIP, stream=stream)
    assert out[0] is Dm and out[1:] == (None, None, None)
    torch.cuda.synchronize()
    what = (N, ncols, c0, b, keep_zero, cap, layouts)
    assert int(read_guarded(tc)[0]) == count, what
    got_first = read_guarded(tf)
    assert np.array_equal(got_first, want.first), (what, np.flatnonzero(got_first != want.first)[:8])
    n = min(count, capn)
    s = read_guarded(ts)
    if src and capn:
        assert np.array_equal(s[:n], want.src[:n]), what
    assert np.all(s[n if src else 0:] == SENT), what       # behind min(count, capacity) src is not touched; a NULL src: nothing is
    if D:
        got = D.read()
        exp = D.with_rows(want.D[:n])
        assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
    P.unchanged()
    if route and N:
        T, plan = T_of(dev), dev.lf1_plan(N, ncols, b)
        fams = ["gf2_lf1_first_kernelILb%d" % (1 if b <= T else 0), "gf2_lf1_count_kernelILi%d" % (plan[3] // 256), "gf2_lf1_scan_kernel"]
        if capn:
            fams.append("gf2_lf1_scatter_kernelILi%dE" % plan[4])   # the first template argument: lanes per row
        assert_route(k0, census(L), fams)
    return want


# ---- window sizes and positions --------------------------------------------------------------------------------------------------

def window_cases():
    try:
        from m4ri_rust_amd import device
        T = T_of(device)
    except Exception:   # not built yet: the fixture builds; test_the_window_cases_are_the_plans checks the list
        T = 14
    bs = sorted({0, 1, 2, T - 1, T, T + 1, 20})
    cases = [(256, c0, b) for b in bs for c0 in (0, 37)]
    cases += [(256, 50, 20),                      # across a word boundary
              (256, 256 - 20, 20), (256, 256 - T, T),      # c0 + b == ncols, a multiple of 64
              (200, 200 - 20, 20), (200, 200 - T, T), (130, 130 - 9, 9),   # ... and not one (130: the window crosses into the short word)
              (256, 64, T), (130, 64, 2), (200, 128, T + 1)]   # from bit 0 of the second / third word
    return cases


WINDOWS = window_cases()


def test_the_window_cases_are_the_plans(dev):
    assert WINDOWS == window_cases()
    T = T_of(dev)
    assert 2 < T < 20 and {b for _, _, b in WINDOWS} >= {0, 1, 2, T - 1, T, T + 1, 20}
    assert dev.lf1_plan(1000, 256, T)[0] == 0 and dev.lf1_plan(1000, 256, T + 1)[0] == 1


@pytest.mark.parametrize("keep_zero", [False, True], ids=["drop", "keep0"])
@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: "%d-c%d-b%d" % c)
def test_windows(dev, L, case, keep_zero):
    ncols, c0, b = case
    N = 3 * R_of(dev, ncols) + 5
    words = pool(N, ncols, c0, b, 100 + c0 + b, classes=700)     # N >> classes: nearly every row survives and has a partner
    set_keys(words[5:9], c0, b, np.zeros(4))                     # some rows of key 0
    want = run(dev, L, words, ncols, c0, b, keep_zero, layouts=(OO, EE) if keep_zero else (EE, OE))
    assert not lf.keys(want.D, c0, b).any()                      # the window of D is zero


def test_class_firsts_of_a_table_of_2_to_24(dev, L):
    """`first` alone, 64 MiB of table: N << 2^b"""
    import torch
    N, ncols, c0, b = 50001, 200, 50, 24
    words = pool(N, ncols, c0, b, 24)
    words[40000:40100] = words[100:200]      # classes of two members: the earlier one wins
    P = View(dev, N, ncols, OO, 24, words)
    tf, pf = guarded(1 << b)
    torch.cuda.synchronize()
    assert dev.class_first(P.m, c0, b, out=pf) is None
    torch.cuda.synchronize()
    want = lf.class_first(words, c0, b)
    got = read_guarded(tf)
    assert np.array_equal(got, want)
    assert (want >= 0).sum() <= N - 100 and want[lf.keys(words[100:101], c0, b)[0]] <= 100
    P.unchanged()
    del tf, got
    gc.collect()
    torch.cuda.empty_cache()


def test_class_first_wrapper_and_small_tables(dev, L):
    T = T_of(dev)
    for b, c0 in ((0, 7), (3, 62), (T, 0), (T + 1, 37)):
        words = pool(5000, 130, c0, b, b, classes=50)
        P = dev.DMat.from_words(words, 130)
        got = dev.class_first(P, c0, b)
        assert got.dtype == np.int32 and np.array_equal(got, lf.class_first(words, c0, b)), b
    # no row: every class is empty
    got = dev.class_first(View(dev, 0, 130, EE, 1).m, 3, 9)
    assert np.array_equal(got, np.full(512, -1))


# ---- row widths and alignment ----------------------------------------------------------------------------------------------------

WIDTHS = [1, 64, 65, 130, 200, 256, 257, 320, 513, 1030, 4100]


def test_the_widths_cover_the_lanes(dev):
    lanes = {dev.lf1_plan(100, n, 4)[4] for n in WIDTHS}
    assert lanes == {dev.lf1_plan(100, n, 4)[4] for n in range(1, 8200, 61)} and len(lanes) >= 3
    assert any(n % 64 for n in WIDTHS) and any(n % 64 == 0 for n in WIDTHS) and any(g.width(n) % 2 for n in WIDTHS)


@pytest.mark.parametrize("layouts", LAYOUT_PAIRS, ids=lambda p: "P%d%d-D%d%d" % (p[0] + p[1]))
@pytest.mark.parametrize("ncols", WIDTHS)
def test_widths_and_alignment(dev, L, ncols, layouts):
    b = min(5, ncols)
    c0 = ncols - b               # the window ends with the row
    N = R_of(dev, ncols) + 77    # two blocks
    words = pool(N, ncols, c0, b, ncols, classes=20)
    words[N - 3] = words[2]      # a repeated row: a zero row in D (unless it leads its class)
    run(dev, L, words, ncols, c0, b, keep_zero=bool(ncols & 1), cap="more", layouts=layouts)
    run(dev, L, words, ncols, c0, b, keep_zero=not (ncols & 1), cap="less", layouts=layouts, src=False)


# ---- row counts ------------------------------------------------------------------------------------------------------------------

def count_cases():
    return [("narrow", n) for n in (0, 1, 2, 63, 64, 65, "R-1", "R", "R+1", "3R+5")] + [("wide", n) for n in ("R-1", "R", "R+1", "3R+5")]


@pytest.mark.parametrize("case", count_cases(), ids=lambda c: "%s-%s" % c)
def test_row_counts(dev, L, case):
    kind, n = case
    ncols = 128 if kind == "narrow" else 320
    R = R_of(dev, ncols)
    N = {"R-1": R - 1, "R": R, "R+1": R + 1, "3R+5": 3 * R + 5}.get(n, n)
    c0, b = 60, 8
    words = pool(N, ncols, c0, b, 900 + N, classes=11)
    want = run(dev, L, words, ncols, c0, b, layouts=(OE, EE))
    if N == 0:
        assert len(want.src) == 0 and np.all(want.first == -1)
    run(dev, L, words, ncols, c0, b, keep_zero=True, cap="equal", layouts=(EE, OO))


def test_more_block_counts_than_one_round_of_the_scan(dev, L):
    ncols, c0, b = 128, 100, 12
    R, chunk = R_of(dev, ncols), scan_chunk()
    N = chunk * R + 2 * R + 5
    assert dev.lf1_plan(N, ncols, b)[5] // 4 > chunk
    words = pool(N, ncols, c0, b, 4242)
    want = run(dev, L, words, ncols, c0, b, layouts=(EE, EE))
    assert len(want.src) == N - (1 << b) and want.src[-1] == N - 1 and (want.src >= chunk * R).sum() > 2 * R


# ---- key distributions -----------------------------------------------------------------------------------------------------------

def T_pair(dev):
    T = T_of(dev)
    return [T, T + 1]


@pytest.mark.parametrize("late", [0, 1], ids=["lds", "global"])
def test_key_distributions(dev, L, late):
    b = T_pair(dev)[late]
    ncols, c0 = 256, 37
    N = 3 * 4096 + 5           # several workgroups of either class-first kernel
    rng = np.random.default_rng(b)
    # one class: every partner is row 0
    words = set_keys(g.random_words(N, ncols, 1), c0, b, np.full(N, 12345 % (1 << b)))
    want = run(dev, L, words, ncols, c0, b)
    assert len(want.src) == N - 1 and not want.partner.any()
    # all keys distinct: nothing survives, nothing is written
    words = set_keys(g.random_words(N, ncols, 2), c0, b, rng.permutation(1 << b)[:N])
    want = run(dev, L, words, ncols, c0, b, cap=7)
    assert len(want.src) == 0
    # random keys, N << 2^b and N >> 2^b
    want = run(dev, L, g.random_words(300, ncols, 3), ncols, c0, b)
    assert len(want.src) < 30
    words = pool(40000, ncols, c0, b, 4, classes=64)
    want = run(dev, L, words, ncols, c0, b, cap="less")
    assert len(want.src) == 40000 - 64
    # repeated identical rows: zero rows in D
    words = np.repeat(g.random_words(9, ncols, 5), 700, axis=0)[rng.permutation(6300)]
    want = run(dev, L, words, ncols, c0, b, layouts=(OO, OO))
    assert len(want.src) == 6300 - 9 and not want.D.any()


@pytest.mark.parametrize("late", [0, 1], ids=["lds", "global"])
def test_the_first_of_a_class_is_its_lowest_row_wherever_it_is_processed(dev, L, late):
    """rows go to the workgroups of the class-first kernel in runs of its 512 threads, round robin: one class has its lowest row in
    the last workgroup and later rows in all the others, one the mirror of it.  A minimum that took "some" row shows in `first`."""
    b = T_pair(dev)[late]
    ncols, c0 = 256, 37
    N = 3 * 4096 + 5
    groups = -(-N // 4096) if late == 0 else -(-N // 512)
    assert groups >= 4
    in_last = [r for r in range(N) if (r // 512) % groups == groups - 1]
    words = pool(N, ncols, c0, b, 77, classes=40)
    used = set(lf.keys(words, c0, b).tolist())
    free = [v for v in range(1 << b) if v not in used][:2]
    # with one pass per workgroup (the global variant here) the last workgroup holds the last rows: the class then starts in the middle
    a0 = in_last[7] if late == 0 else 5000
    a_rows = [a0, a0 + 512 + 3, a0 + 2 * 512 + 1, N - 3]
    b_rows = [3, 512 + 5, in_last[-1]]
    assert a_rows == sorted(a_rows) and b_rows == sorted(b_rows) and not set(a_rows) & set(b_rows)
    assert late or len({(r // 512) % groups for r in a_rows[:3]}) == 3
    for rows, v in ((a_rows, free[0]), (b_rows, free[1])):
        for r in rows:
            set_keys(words[r:r + 1], c0, b, [v])
    want = run(dev, L, words, ncols, c0, b)
    assert want.first[free[0]] == a_rows[0] and want.first[free[1]] == 3
    for rows in (a_rows, b_rows):
        at = [list(want.src).index(r) for r in rows[1:]]
        assert all(want.partner[i] == rows[0] for i in at)


# ---- flags and capacity ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keep_zero", [False, True], ids=["drop", "keep0"])
@pytest.mark.parametrize("zeros", ["none", "some", "only"])
def test_keep_zero(dev, L, zeros, keep_zero):
    N, ncols, c0, b = 3000, 200, 120, 10     # the window crosses from word 1 into word 2
    words = pool(N, ncols, c0, b, 31, classes=25)
    k = lf.keys(words, c0, b)
    if zeros == "none":
        set_keys(words, c0, b, np.where(k == 0, 1, k))
    elif zeros == "some":
        set_keys(words[100:400], c0, b, np.zeros(300))
    else:
        set_keys(words, c0, b, np.zeros(N))
    want = run(dev, L, words, ncols, c0, b, keep_zero, layouts=(EO, EE))
    nz = int((lf.keys(words, c0, b) == 0).sum())
    assert (nz == 0) == (zeros == "none") and (nz == N) == (zeros == "only")
    if keep_zero and nz:
        kept = want.partner < 0
        assert kept.sum() == nz and np.array_equal(want.D[kept], words[want.src[kept]])    # unchanged, the first of them included
    if zeros == "only":
        assert len(want.src) == (N if keep_zero else N - 1)


@pytest.mark.parametrize("src", [True, False], ids=["src", "nosrc"])
@pytest.mark.parametrize("cap", ["zero", "less", "equal", "more", 1])
def test_capacity(dev, L, cap, src):
    N, ncols, c0, b = 2500, 257, 250, 7
    words = pool(N, ncols, c0, b, 55)
    want = run(dev, L, words, ncols, c0, b, cap=cap, src=src, layouts=(OO, OE))
    assert len(want.src) == N - 128


def test_wrapper_sizes_the_result(dev):
    N, ncols, c0, b = 5000, 100, 41, 6
    words = pool(N, ncols, c0, b, 8)
    want = lf.lf1(words, ncols, c0, b)
    P = dev.DMat.from_words(words, ncols)
    D, count, first, src = dev.lf1_reduce(P, c0, b)          # cap=None: a count-only call first
    assert D.nrows == len(want.src) == N - 64 and np.array_equal(D.to_words(), want.D)
    assert int(count.read(None)[0]) == D.nrows and np.array_equal(first.read(None), want.first) and np.array_equal(src.read(None), want.src)
    D = P.lf1_reduce(c0, b, keep_zero=True)
    wz = lf.lf1(words, ncols, c0, b, True)
    assert D.nrows == len(wz.src) and np.array_equal(D.to_words(), wz.D)
    # nothing survives: an empty matrix
    E = dev.DMat.from_words(words[:1], ncols).lf1_reduce(c0, b)
    assert E.nrows == 0 and E.ncols == ncols
    assert np.array_equal(P.to_words(), words)


# ---- dirty scratch, streams ------------------------------------------------------------------------------------------------------

def test_on_dirty_scratch(dev, L):
    """the block counts come from a cache in which every block holds a pattern, and no block comes fresh from the driver"""
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for N, ncols, b in ((3 * R_of(dev, 128) + 5, 128, 6), (100003, 320, T_of(dev) + 1)):
            words = pool(N, ncols, 33, b, N, classes=300)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run(dev, L, words, ncols, 33, b, keep_zero=True, stream=stream)
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the LF1 round on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pool is written by gf2_dmat_fill_random on the caller's stream, behind a sleep; the same round is enqueued twice behind it,
    into two destinations, before anything synchronises.  Both must hold what the reference makes of the seeded pool."""
    import torch
    N, ncols, c0, b, seed = 20011, 200, 57, 9, 0xB1C
    words = lr.seeded_words(seed, ncols, np.arange(N))
    want = lf.lf1(words, ncols, c0, b)
    count = len(want.src)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    tp = torch.full((N, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    P = dev.DMat.from_torch(tp, ncols)
    outs = []
    for _ in range(2):
        td = torch.full((count + 2, 4), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.from_torch(td, ncols), guarded(1 << b), guarded(1), guarded(count + 2)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    P.fill_random(seed, s)
    for td, D, (tf, pf), (tc, pc), (ts, ps) in outs:
        dev.lf1_reduce(P, c0, b, D=D, first=pf, count=pc, src=ps, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    results = []
    for td, D, (tf, pf), (tc, pc), (ts, ps) in outs:
        rows = td.cpu().numpy().view(np.uint64)
        assert int(read_guarded(tc)[0]) == count
        assert np.array_equal(rows[:count], want.D) and np.all(rows[count:] == np.uint64(0x1111111111111111))
        assert np.array_equal(read_guarded(tf), want.first) and np.array_equal(read_guarded(ts)[:count], want.src)
        results.append((rows, read_guarded(tf), read_guarded(ts)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))


# ---- past 4 GiB, composition, end to end -----------------------------------------------------------------------------------------

def test_a_view_of_a_parent_past_4gib(dev, L):
    """70 000 rows of 128 columns, 8192 words apart: the last rows start behind byte offset 2^32 of the parent.  Only the view's words
    are written (gf2_copy_block_dev from a compact upload); D is compact"""
    import torch
    N, ncols, ld, c0, b = 70000, 128, 8192, 60, 10
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((N, ld), dtype=torch.int64, device="cuda")
    assert N * ld * 8 > lr.LIMIT_BYTES
    words = pool(N, ncols, c0, b, 70)
    r_hi = lr.straddle(ld, N)[1]
    k = lf.keys(words, c0, b)
    set_keys(words[5:6], c0, b, [k[0] ^ 1 if k[0] ^ 1 not in k[1:5] else k[0] ^ 2])   # row 5 leads its class ...
    assert lf.keys(words[5:6], c0, b)[0] not in lf.keys(words[:5], c0, b)
    words[N - 1] = words[5]                       # ... and the last row repeats it: a pair on either side of 2^32
    P = dev.DMat.wrap(t.data_ptr() + 8 * 6, N, ncols, ld, keep=t)
    dev.copy_block(P, 0, 0, dev.DMat.from_words(words, ncols), 0, 0, N, ncols)
    want = lf.lf1(words, ncols, c0, b)
    D, count, first, src = dev.lf1_reduce(P, c0, b, cap=len(want.src) + 1)
    assert int(count.read(None)[0]) == len(want.src)
    assert np.array_equal(first.read(None), want.first)
    assert np.array_equal(src.read(None)[:-1], want.src)
    assert np.array_equal(D.to_words()[:-1], want.D)
    assert (want.src > r_hi).sum() > 0 and not want.D[list(want.src).index(N - 1)].any()
    del t, P, D
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("keep_zero", [False, True], ids=["drop", "keep0"])
def test_the_index_outputs_feed_the_gathers(dev, keep_zero):
    """D == gather(P, src) ^ gather(P, first[key(src)]): src goes to the gather as the device array it is, the partners are uploaded
    from the reference (-1, a kept row of key 0: the accumulating gather leaves the row)"""
    N, ncols, c0, b = 9000, 300, 100, 8
    words = pool(N, ncols, c0, b, 17)
    want = lf.lf1(words, ncols, c0, b, keep_zero)
    P = dev.DMat.from_words(words, ncols)
    D, count, first, src = dev.lf1_reduce(P, c0, b, keep_zero=keep_zero, cap=len(want.src))
    D2 = dev.DMat(len(want.src), ncols)
    dev.gather_rows(P, src.ptr, D=D2)
    dev.gather_rows(P, want.partner, D=D2, accumulate=True)
    assert np.array_equal(D2.to_words(), want.D) and np.array_equal(D.to_words(), want.D)
    assert np.array_equal(want.first[lf.keys(words[want.src], c0, b)][want.partner >= 0], want.partner[want.partner >= 0])


def lpn_samples(seed, N=4096, k=16, tau=1 / 16):
    rng = np.random.default_rng(seed)
    secret = rng.integers(0, 2, k, dtype=np.uint8)
    samples = rng.integers(0, 2, (N, k), dtype=np.uint8)
    errors = (rng.random(N) < tau).astype(np.uint8)
    label = (samples.astype(np.int64) @ secret.astype(np.int64) + errors) % 2
    bits = np.concatenate([samples, label[:, None].astype(np.uint8)], axis=1)
    return g.bits_to_words(bits), secret


def bkw_reference(words):
    """two LF1 rounds and the error counts of all 2^8 secrets, in numpy"""
    r1 = lf.lf1(words, 17, 12, 4)
    r2 = lf.lf1(r1.D, 17, 8, 4)
    bits = g.words_to_bits(r2.D, 17).astype(np.int64)
    s = (np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1
    errors = ((bits[:, :8] @ s.T) % 2 != bits[:, 16:17]).sum(axis=0)
    return r1, r2, bits, errors


@pytest.mark.parametrize("seed", [0, 7, 19])
def test_bkw_end_to_end(dev, seed):
    """k = 16, N = 4096, noise 1/16: two rounds of 4 bits, the errors of the 2^8 secrets that are left, the minimum -- one chain, one
    synchronisation at its end"""
    import torch
    words, secret = lpn_samples(seed)
    r1, r2, bits, errors = bkw_reference(words)
    assert r1.D.shape[0] == 4080 and r2.D.shape[0] == 4064 and not bits[:, 8:16].any()
    low = int(sum(int(x) << j for j, x in enumerate(secret[:8])))
    order = np.argsort(errors, kind="stable")
    assert order[0] == low and errors[order[0]] <= 1511 and errors[order[1]] >= 1911    # the reference recovers the secret (seeds 0..19)
    P = dev.DMat.from_words(words, 17)
    te, pe = guarded(256)
    tm, pm = guarded(2)
    torch.cuda.synchronize()
    D1, c1, _, _ = dev.lf1_reduce(P, 12, 4, cap=4080, src=dev.SKIP)
    D2, c2, _, _ = dev.lf1_reduce(D1, 8, 4, cap=4064, src=dev.SKIP)
    dev.lpn_errors(D2, 0, 8, 16, out=pe)
    dev.min_weight(pe, 256, idx=pm, val=pm + 4)
    torch.cuda.synchronize()
    assert int(c1.read(None)[0]) == 4080 and int(c2.read(None)[0]) == 4064
    assert np.array_equal(D1.to_words(), r1.D) and np.array_equal(D2.to_words(), r2.D)
    assert np.array_equal(read_guarded(te), errors)
    assert list(read_guarded(tm)) == [low, int(errors[low])]
    # the method of the matrix gives the same pools
    Q = P.lf1_reduce(12, 4).lf1_reduce(8, 4)
    assert Q.nrows == 4064 and np.array_equal(Q.to_words(), r2.D)
    assert np.array_equal(Q.lpn_errors(0, 8, 16), errors)
