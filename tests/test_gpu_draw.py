"""GPU tests of include/m4ri_hip_draw.h: gf2_bernoulli_dev / gf2_bernoulli_block_dev, gf2_draw_indices_dev, gf2_draw_subsets_dev and
gf2_draw_permutation_dev bit for bit against the yardstick of tests/draw_ref.py (itself checked against the published known answers
and the per-bit definitions by tests/test_draw_reference.py; the shipped per-word functions against it by
tests/test_draw_philox_cpu.py).

A Bernoulli destination is a window of a dirty parent in the layouts of tests/dev_views.py -- here the window and the excess bits of
its last word are dirty too -- and the whole parent is compared afterwards: a store outside the rows' words, an excess bit that is
not zero (accumulate == 0) or not kept (accumulate == 1) fails the case.  The int outputs lie between sentinels and hold a pattern
before the call.  Lanes per pass of the grid, subsets per workgroup and the scratch are read from gf2_draw_plan, never written down
here; which kernels ran is read from the launch census."""
import functools
import gc

import numpy as np
import pytest

import dev_views as dv
import dirty_pool as dp
import draw_ref as dr
import gf2util as g
import limits_ref as lr
from census_util import assert_route, census

pytestmark = pytest.mark.gpu

SENT = 0x5EAD5EAD    # what an int output holds before the call
THRS = [0, 1, 0x20000000, 0x80000000, 0x12345679, 0xFFFFFFFF]      # no plane, all sixteen calls, two, one, sixteen, all ones
SORT = ["gf2_lf2_sort_count_kernel", "gf2_lf2_scan_sums_kernel", "gf2_lf2_scan_group_kernelIi", "gf2_lf2_scan_apply_kernel",
        "gf2_lf2_sort_scatter_kernel"]


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


def guarded(n, shift=0):
    """n device ints between sentinels, all holding SENT; -> (tensor, address of the n ints); shift = 1: an address that is only
    4-byte aligned"""
    import torch
    t = torch.full((n + 8 + shift,), SENT, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 16 + 4 * shift


def read_guarded(t, shift=0):
    h = t.cpu().numpy()
    assert np.all(h[:4 + shift] == SENT) and np.all(h[-4:] == SENT), "a word next to an int output was written"
    return h[4 + shift:-4]


@functools.lru_cache(maxsize=None)
def noise(seed, thr, nrows, ncols, row0=0, col_word0=0, full_ncols=0):
    words = dr.bernoulli(seed, thr, nrows, ncols, row0, col_word0, full_ncols)
    words.setflags(write=False)
    return words


class DirtyWindow:
    """nrows x ncols in a layout of tests/dev_views.py; every word of the parent is random, the window and its excess bits included"""

    def __init__(self, dev, nrows, ncols, layout, seed):
        import torch
        self.ld, self.cw = dv.geometry(ncols, layout)
        self.w = g.width(ncols)
        self.nrows, self.ncols = nrows, ncols
        self.host = np.random.default_rng(seed).integers(0, 1 << 64, (dv.R0 + nrows + dv.BELOW, self.ld), dtype=np.uint64)
        self.t = torch.from_numpy(self.host.view(np.int64).copy()).cuda()
        self.base = self.t.data_ptr() + 8 * (dv.R0 * self.ld + self.cw)
        assert self.t.data_ptr() % 16 == 0
        self.m = dev.DMat.wrap(self.base, nrows, ncols, self.ld, keep=self.t)
        self.vec = self.w > 1 and self.base % 16 == 0 and (self.ld % 2 == 0 or nrows == 1)     # the rule of the header

    def read(self):
        return self.t.cpu().numpy().view(np.uint64).reshape(self.host.shape)

    def expect(self, words, accumulate):
        want = self.host.copy()
        win = want[dv.R0:dv.R0 + self.nrows, self.cw:self.cw + self.w]
        win[...] = win ^ words if accumulate else words
        return want


def bernoulli_kernel(vec):
    return "gf2_bernoulli_kernelILi%dE" % (2 if vec else 1)


# ---- Bernoulli ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", dv.LAYOUTS)
@pytest.mark.parametrize("shape", [(1, 1), (3, 65), (70, 129)], ids=lambda s: "%dx%d" % s)
def test_bernoulli_on_dirty_views(dev, L, shape, layout):
    import torch
    nrows, ncols = shape
    seed = 1000 * nrows + ncols
    for thr in THRS:
        want = noise(seed, thr, nrows, ncols)
        assert not (ncols % 64 and (want[:, -1] >> np.uint64(ncols % 64)).any())
        for accumulate in (0, 1):
            V = DirtyWindow(dev, nrows, ncols, layout, seed + accumulate)
            torch.cuda.synchronize()
            k0 = census(L)
            assert dev.bernoulli(V.m, thr, seed, accumulate=accumulate) is V.m
            torch.cuda.synchronize()
            got, exp = V.read(), V.expect(want, accumulate)
            what = (shape, layout, hex(thr), accumulate)
            assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
            if thr:
                assert_route(k0, census(L), [bernoulli_kernel(V.vec)])
            else:
                assert census(L) == k0, what      # no Philox call: no kernel
    assert DirtyWindow(dev, nrows, ncols, layout, 0).vec == (ncols > 64 and layout in (dv.EE, dv.WIDE))


def test_bernoulli_density(dev):
    """tau = 1/8 and tau = 0x12345679 / 2^32 over 2^20 bits: within five standard deviations"""
    for thr in (0x20000000, 0x12345679):
        D = dev.DMat(1024, 1024).bernoulli_(thr, 31)
        p = thr / 2 ** 32
        assert abs(D.count_ones() - p * 2 ** 20) < 5 * np.sqrt(2 ** 20 * p * (1 - p))
        assert np.array_equal(D.to_words(), noise(31, thr, 1024, 1024))
        assert not np.array_equal(dev.DMat(1024, 1024).bernoulli_(thr, 32).to_words(), noise(31, thr, 1024, 1024))     # another seed


@pytest.mark.parametrize("layout", [dv.EE, dv.OO])
def test_a_block_is_the_same_rectangle_of_the_whole(dev, L, layout):
    import torch
    seed, thr, rows, cols = 77, 0x12345679, 40, 640
    whole = dev.DMat(rows, cols).bernoulli_(thr, seed).to_words()
    assert np.array_equal(whole, noise(seed, thr, rows, cols))
    for ncols, accumulate in ((128, 0), (100, 0), (100, 1), (64, 1)):
        w = g.width(ncols)
        rect = whole[11:18, 3:3 + w].copy()
        if ncols % 64:
            rect[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
        assert np.array_equal(rect, noise(seed, thr, 7, ncols, 11, 3, cols))
        V = DirtyWindow(dev, 7, ncols, layout, ncols + accumulate)
        dev.bernoulli(V.m, thr, seed, accumulate=accumulate, row0=11, col_word0=3, full_ncols=cols)
        torch.cuda.synchronize()
        assert np.array_equal(V.read(), V.expect(rect, accumulate)), (ncols, accumulate, layout)
    # row0 alone: the rows of a taller matrix of the same width
    V = DirtyWindow(dev, 5, cols, layout, 5)
    dev.bernoulli(V.m, thr, seed, row0=20)
    torch.cuda.synchronize()
    assert np.array_equal(V.read(), V.expect(whole[20:25], 0))


@pytest.mark.parametrize("vec", [True, False], ids=["16-byte", "8-byte"])
def test_more_words_than_one_pass_of_the_grid(dev, L, vec):
    import torch
    lanes = dev.draw_plan("bernoulli", thr=0x20000000)[2]
    w = 1001
    ld = w + 1 if vec else w                     # an odd stride: no 16-byte store
    nrows = lanes // ((w + 1) // 2 if vec else w) + 30
    assert nrows * ((w + 1) // 2 if vec else w) > lanes and nrows * ld * 8 < 32 << 20
    t = torch.full((nrows, ld), 0x1111111111111111, dtype=torch.int64, device="cuda")
    D = dev.DMat.wrap(t.data_ptr(), nrows, 64 * w - 5, ld, keep=t)
    k0 = census(L)
    dev.bernoulli(D, 0x20000000, 12)
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:, :w], noise(12, 0x20000000, nrows, 64 * w - 5))
    assert np.all(got[:, w:] == np.uint64(0x1111111111111111))
    assert_route(k0, census(L), [bernoulli_kernel(vec)])


def test_the_word_index_crosses_2_to_32(dev):
    """three rows of a matrix of 1024 words per row from row 2^22 - 1 on: the second row starts with word 2^32, counter word 1"""
    import torch
    row0, cols = (1 << 22) - 1, 64 * 1024
    want = noise(3, 0x12345679, 3, cols, row0, 0, cols)
    assert np.array_equal(want[1, :2], dr.bernoulli_words(3, [1 << 32, (1 << 32) + 1], 0x12345679)[0])
    assert not np.array_equal(want[1], noise(3, 0x12345679, 1, cols)[0])       # not the words 0, 1, ...
    D = dev.DMat(3, cols)
    dev.bernoulli(D, 0x12345679, 3, row0=row0, full_ncols=cols)
    assert np.array_equal(D.to_words(), want)
    V = DirtyWindow(dev, 2, 64, dv.OO, 9)                   # the last word of two rows: words 2^32 - 1 and 2^32 + 1023
    dev.bernoulli(V.m, 0x80000000, 3, accumulate=True, row0=row0, col_word0=1023, full_ncols=cols)
    torch.cuda.synchronize()
    rect = noise(3, 0x80000000, 2, 64, row0, 1023, cols)
    assert np.array_equal(rect[:, 0], dr.bernoulli_words(3, np.array([(1 << 32) - 1, (1 << 32) + 1023], dtype=np.uint64), 0x80000000)[0])
    assert np.array_equal(V.read(), V.expect(rect, 1))


# ---- indices -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 1000, (1 << 31) - 1])
def test_indices(dev, L, n):
    import torch
    for count in (1, 63, 64, 65, 1001):
        for shift in (0, 1):
            t, p = guarded(count, shift)
            torch.cuda.synchronize()
            k0 = census(L)
            assert dev.draw_indices(count, n, 40 + count, out=p) is None
            torch.cuda.synchronize()
            got = read_guarded(t, shift)
            assert np.array_equal(got, dr.indices(40 + count, count, n)), (count, n, shift)
            assert_route(k0, census(L), ["gf2_draw_indices_kernel"])
    t, p = guarded(4)
    dev.draw_indices(0, n, 1, out=p)
    torch.cuda.synchronize()
    assert np.all(read_guarded(t) == SENT)


def test_more_indices_than_one_pass_of_the_grid_feed_the_gather(dev, L):
    draws = dev.draw_plan("indices", 1, 1)[2]
    count, n = draws + 12345, 5000
    idx = dev.draw_indices(count, n, 8)
    want = dr.indices(8, count, n)
    assert np.array_equal(idx.read(None), want)
    words = g.random_words(n, 100, 4)
    D, _ = dev.gather_rows(dev.DMat.from_words(words, 100), idx.ptr, D=dev.DMat(2000, 100))
    assert np.array_equal(D.to_words(), words[want[:2000]])
    assert len(dev.draw_indices(0, n, 8).read(None)) == 0


# ---- subsets -----------------------------------------------------------------------------------------------------------------------------

SUBSETS = [(1, 2), (2, 4), (8, 16), (64, 128), (65, 130), (512, 1024), (1024, 2048), (64, 1 << 20)]


@pytest.mark.parametrize("many", [False, True], ids=["one", "many"])
@pytest.mark.parametrize("case", SUBSETS, ids=lambda c: "%d-of-%d" % c)
def test_subsets(dev, L, case, many):
    import torch
    k, n = case
    batch = (1000 if k <= 65 else 3) if many else 1
    seed = 7 * k + n
    want, unfinished = dr.subsets(seed, batch, k, n)
    assert unfinished == 0 and want.min() >= 0
    t, p = guarded(batch * k)
    tu, pu = guarded(1)
    torch.cuda.synchronize()
    k0 = census(L)
    assert dev.draw_subsets(batch, k, n, seed, out=p, unfinished=pu) == (None, None)
    torch.cuda.synchronize()
    got = read_guarded(t).reshape(batch, k)
    assert got.min() >= 0 and got.max() < n and all(len(set(row)) == k for row in got)       # in range, distinct
    assert np.array_equal(got, want), (case, batch, np.argwhere(got != want)[:8])
    assert list(read_guarded(tu)) == [0]
    per_group = dev.draw_plan("subsets", k, n)[2]
    assert (per_group > 1) == (k <= 64)
    assert_route(k0, census(L), ["gf2_draw_subsets_kernelILb%dE" % (1 if per_group > 1 else 0)])


@pytest.mark.parametrize("case", [(8, 16, 1000, 1), (8, 16, 1000, 2), (65, 130, 50, 1), (1024, 2048, 2, 3)], ids=lambda c: "%d-of-%d-x%d-r%d" % c)
def test_a_short_max_rounds_leaves_minus_one(dev, L, case):
    import torch
    k, n, batch, rounds = case
    want, unfinished = dr.subsets(5, batch, k, n, max_rounds=rounds)
    assert 0 < unfinished <= batch and (want < 0).any()
    t, p = guarded(batch * k)
    tu, pu = guarded(1)
    dev.draw_subsets(batch, k, n, 5, max_rounds=rounds, out=p, unfinished=pu)
    torch.cuda.synchronize()
    got = read_guarded(t).reshape(batch, k)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert list(read_guarded(tu)) == [unfinished]
    # unfinished may be NULL; the wrapper's own arrays
    t, p = guarded(batch * k)
    dev.draw_subsets(batch, k, n, 5, max_rounds=rounds, out=p, unfinished=dev.SKIP)
    torch.cuda.synchronize()
    assert np.array_equal(read_guarded(t).reshape(batch, k), want)
    sub, unf = dev.draw_subsets(batch, k, n, 5, max_rounds=rounds)
    assert np.array_equal(sub.read(None).reshape(batch, k), want) and list(unf.read(None)) == [unfinished]


def test_no_subset(dev):
    import torch
    t, p = guarded(4)
    tu, pu = guarded(1)
    dev.draw_subsets(0, 8, 16, 1, out=p, unfinished=pu)
    torch.cuda.synchronize()
    assert np.all(read_guarded(t) == SENT) and list(read_guarded(tu)) == [0]      # only *unfinished is written


# ---- permutation -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 70000])
def test_permutation(dev, L, n):
    import torch
    want = dr.permutation(n + 1, n)
    if n == 70000:
        keys = dr.perm_keys(n + 1, n)
        assert len(np.unique(keys)) < n           # ties: they fall in index order
    t, p = guarded(n)
    torch.cuda.synchronize()
    k0 = census(L)
    assert dev.draw_permutation(n, n + 1, out=p) is None
    torch.cuda.synchronize()
    got = read_guarded(t)
    assert np.array_equal(np.sort(got), np.arange(n))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert_route(k0, census(L), ["gf2_draw_perm_pairs_kernel"] + SORT)


def test_the_permutation_feeds_the_gathers(dev):
    import torch
    n = 300
    words = g.random_words(50, n, 6)
    perm = dev.draw_permutation(n, 3)
    want = dr.permutation(3, n)
    assert np.array_equal(perm.read(None), want)
    D, _ = dev.gather_cols(dev.DMat.from_words(words, n), perm.ptr, D=dev.DMat(50, n))
    assert np.array_equal(D.to_words(), g.bits_to_words(g.words_to_bits(words, n)[:, want]))
    t, p = guarded(4)
    dev.draw_permutation(0, 3, out=p)
    torch.cuda.synchronize()
    assert np.all(read_guarded(t) == SENT)
    assert len(dev.draw_permutation(0, 3).read(None)) == 0


def test_permutation_behind_pending_work_on_dirty_scratch(dev, L):
    """the pair buffers and digit counts come from a cache in which every block holds a pattern and no block comes fresh from the
    driver; the call is enqueued twice on a caller stream behind a sleep, into two arrays, before anything synchronises"""
    import torch
    n, seed = 70000, 11
    want = dr.permutation(seed, n)
    assert dev.draw_plan("permutation", n=n)[0] < 8 * dp.MIB
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        stream = torch.cuda.Stream()             # a caller stream: its arena is new
        outs = [guarded(n), guarded(n)]
        torch.cuda.synchronize()
        h0 = cache.hits()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(100_000_000)
        for _, p in outs:
            dev.draw_permutation(n, seed, out=p, stream=stream.cuda_stream)
        pending = not stream.query()
        torch.cuda.synchronize()
        assert pending, "the stream had drained before the calls were issued"
        for t, _ in outs:
            assert np.array_equal(read_guarded(t), want)
        assert cache.hits() - h0 >= 1
        cache.no_fresh("the permutation on dirty scratch")
    gc.collect()
    L.gf2_trim()


# ---- the oracle, end to end --------------------------------------------------------------------------------------------------------------

def oracle_pool(seed, N, k, secret, thr):
    """what device.lpn_samples makes, in numpy -> (N x (k + 1) words, the noise bits)"""
    A = lr.seeded_words(seed, k, np.arange(N))
    bits = g.words_to_bits(A, k).astype(np.int64)
    e = (noise(seed, thr, N, 1)[:, 0] & np.uint64(1)).astype(np.int64)
    y = (bits @ np.asarray(secret, dtype=np.int64) + e) % 2
    return g.bits_to_words(np.concatenate([bits, y[:, None]], axis=1).astype(np.uint8)), e


def test_lpn_samples(dev):
    N, k, thr, seed = 4096, 100, 0x20000000, 17
    secret = np.random.default_rng(1).integers(0, 2, k)
    want, e = oracle_pool(seed, N, k, secret, thr)
    assert abs(int(e.sum()) - N / 8) < 5 * np.sqrt(N * 7 / 64)
    P = dev.lpn_samples(N, k, secret, thr, seed)
    assert (P.nrows, P.ncols) == (N, k + 1)
    got = P.to_words()
    assert np.array_equal(got[:, 0], want[:, 0])                                              # the samples: the uniform fill
    assert np.array_equal(g.words_to_bits(got, k + 1)[:, k], g.words_to_bits(want, k + 1)[:, k])    # the labels: A s ^ noise
    assert np.array_equal(got, want)
    s = dev.DMat.from_words(secret.astype(np.uint64).reshape(k, 1), 1)                      # the secret on the device already
    assert np.array_equal(dev.lpn_samples(N, k, s, thr, seed).to_words(), want)


def test_pooled_gauss_round_with_no_host_step(dev):
    """k = 32, N = 4096, tau = 1/16, 256 guesses: draw_subsets, gather_rows, echelonize_batch and the weight verdict of
    INTEGRATION.md section 4 in one chain, one synchronisation at its end.  Candidate b is column k of the echelon form of guess b;
    E = pool * [S ; 1] counts in column b the samples it gets wrong, and the candidates below 2 tau N are selected."""
    import torch
    k, N, thr, batch, seed, limit = 32, 4096, 1 << 28, 256, 2026, 512
    secret = np.random.default_rng(5).integers(0, 2, k)
    pool, e = oracle_pool(seed, N, k, secret, thr)
    sub, unfinished = dr.subsets(seed + 1, batch, k, N)
    assert unfinished == 0
    # the yardstick's round
    bits = g.words_to_bits(pool, k + 1).astype(np.int64)
    stack = np.empty((batch * k, 1), dtype=np.uint64)
    ranks, cands = [], np.zeros((batch, k), dtype=np.int64)
    for b in range(batch):
        red, rank, _ = g.o_echelonize(pool[sub[b]], k, k + 1, full=True, limit=k)
        stack[b * k:(b + 1) * k] = red
        ranks.append(rank)
        cands[b] = (red[:, 0] >> np.uint64(k)) & np.uint64(1)
    clean = [b for b in range(batch) if ranks[b] == k and not e[sub[b]].any()]
    assert len(clean) >= 1, "the seed gives no noise-free guess of full rank"
    assert all(np.array_equal(cands[b], secret) for b in clean)
    weights = ((bits @ np.concatenate([cands.T, np.ones((1, batch), dtype=np.int64)])) % 2).sum(axis=0)
    # the device packs candidates 0, 2, 4, ... in front of 1, 3, 5, ... (two candidates of 32 bits per word of the flat column)
    order = np.concatenate([np.arange(0, batch, 2), np.arange(1, batch, 2)])
    selected = np.flatnonzero(weights[order] <= limit)
    assert set(order[selected]) >= set(clean) and weights[clean[0]] == e.sum() < limit < weights[order].max()
    # the device's
    P = dev.lpn_samples(N, k, secret, thr, seed)
    ones = dev.DMat.from_words(np.full((1, batch // 64), ~np.uint64(0), dtype=np.uint64), batch)
    ts, ps = guarded(batch * k)
    tr, pr = guarded(batch)
    tw, pw = guarded(batch)
    tf, pf = guarded(batch)
    tc, pc = guarded(1)
    torch.cuda.synchronize()
    dev.draw_subsets(batch, k, N, seed + 1, out=ps, unfinished=dev.SKIP)
    Ay, _ = dev.gather_rows(P, ps, D=dev.DMat(batch * k, k + 1))
    dev.echelonize_batch(Ay, k, full=True, ncols_limit=k, ranks=pr, pivots=dev.SKIP)
    flat = dev.transpose(dev.submatrix(Ay, 0, k, batch * k, k + 1))                          # 1 x batch k: the candidates in a row
    two = dev.DMat.wrap(flat.s.data, batch * k // 64, 64, 1, keep=flat)                     # two candidates per row
    St = dev.stack(dev.submatrix(two, 0, 0, two.nrows, k), dev.submatrix(two, 0, k, two.nrows, 2 * k))
    S1 = dev.stack(dev.transpose(St), ones)
    E = dev.mul(P, S1)
    dev.col_weights(E, out=pw)
    dev.select_weights(pw, batch, 0, limit, idx=pf, cap=batch, count=pc)
    torch.cuda.synchronize()
    assert np.array_equal(P.to_words(), pool)
    assert np.array_equal(read_guarded(ts).reshape(batch, k), sub)
    assert np.array_equal(Ay.to_words(), stack) and list(read_guarded(tr)) == ranks
    assert np.array_equal(read_guarded(tw), weights[order])
    count = int(read_guarded(tc)[0])
    found = read_guarded(tf)[:count]
    assert count == len(selected) and np.array_equal(found, selected)                         # exactly the yardstick's candidates
    got = g.words_to_bits(St.to_words(), k)[found]
    assert any(np.array_equal(row, secret) for row in got)                                   # the secret is among them
