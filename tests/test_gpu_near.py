"""GPU tests of include/m4ri_hip_near.h: gf2_near_pairs_dev and gf2_nearest_dev bit for bit against the numpy yardstick of
tests/near_ref.py (itself checked against the definition by tests/test_near_reference.py): the rows of D that are written, the rest of
D, the words around D, `hits`, `ia`, `ib` and `wt` up to min(hits, capacity), `idx` and `dist`.

The harness is that of tests/test_gpu_join_select.py: every operand is a window of a dirty parent (View of tests/test_gpu_lf1.py: the
excess bits of the last word are dirty too) and the whole parent of D is compared afterwards; the int outputs lie between sentinels
and hold a pattern before the call; A and B are unchanged afterwards; the launch census is checked per call.

The block of rows of A, the tile and the chunks of B are read from gf2_near_plan, never written down here; which kernels ran is read
from the launch census.  Every kernel instance of gf2_near.hip is launched by test_widths_and_alignment."""
import functools
import gc
import itertools

import numpy as np
import pytest

import dev_views as dv
import dirty_pool as dp
import gf2util as g
import limits_ref as lr
import near_ref as nr
from census_util import assert_route, census
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded

pytestmark = pytest.mark.gpu

ARRAYS = ("ia", "ib", "wt")
OFF, UPPER = nr.OFF_DIAGONAL, nr.UPPER
LAYOUTS = [(EE, EE, EE), (OO, EO, OE), (EO, OE, OO), (OE, OO, EO)]


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


def capacity(cap, hits):
    return {"zero": 0, "less": hits // 2, "equal": hits, "more": hits + 7}[cap] if isinstance(cap, str) else cap


def median_window(wa, wb, ncols, wcols, flags=0):
    """a window that about half the admitted pairs meet: from 0 to the median distance"""
    if not len(wa) or not len(wb):
        return (0, 0)
    d = nr.distances(wa, wb, ncols, *wcols)[nr.admitted(len(wa), len(wb), flags)]
    return (0, int(np.median(d))) if len(d) else (0, 0)


def launched(before, after, family):
    return any(family in k and v > before.get(k, 0) for k, v in after.items())


def family(plan, mode):
    return "gf2_near_kernelILi%dELi%dEE" % (plan[0], mode) if plan[0] else "gf2_near_wide_kernelILi%dEE" % mode


def run_pairs(dev, L, wa, wb, ncols, wcols, win, flags=0, cap="more", given=ARRAYS, store=True, layouts=(EE, EE, EE), stream=None, same=False,
              want=None):
    """one gf2_near_pairs_dev call on dirty windows against the yardstick -> (the yardstick's result, the hits that were written).
    store=False: D comes without data.  same: B is the view that A is"""
    import torch
    NA, NB = wa.shape[0], wb.shape[0]
    (wc0, wc1), (wlo, whi) = wcols, win
    if want is None:
        want = nr.near_pairs(wa, wb, ncols, wc0, wc1, wlo, whi, flags)
    capn = capacity(cap, want.hits)
    n = min(want.hits, capn)
    A = View(dev, NA, ncols, layouts[0], 11 * NA + wc0, wa)
    B = A if same else View(dev, NB, ncols, layouts[1], 7 * NB + wc1 + 1, wb)
    D = View(dev, capn, ncols, layouts[2], 13 * NA + 5) if capn and store else None
    Dm = D.m if D else dev.DMat.wrap(None, capn, ncols, max(g.width(ncols), 1))
    th, ph = guarded(2)
    ints = {name: guarded(max(capn, 1)) for name in ARRAYS}
    args = {name: ints[name][1] if name in given and capn else dev.SKIP for name in ARRAYS}
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.near_pairs(A.m, B.m, (wc0, wc1), wlo, whi, flags=flags, D=Dm if store or not capn else None, cap=capn, store=store or not capn,
                         hits=ph, stream=stream, **args)
    assert out[0] is (Dm if store or not capn else None) and out[1:] == (None,) * 4
    torch.cuda.synchronize()
    k1 = census(L)
    what = (NA, NB, ncols, (wc0, wc1), (wlo, whi), flags, cap, given, store, layouts)
    assert int(read_guarded(th).view(np.int64)[0]) == want.hits, what
    for name, rows in (("ia", want.ia), ("ib", want.ib), ("wt", want.wt)):
        a = read_guarded(ints[name][0])
        written = name in given and capn
        if written:
            assert np.array_equal(a[:n], rows[:n]), (what, name, np.flatnonzero(a[:n] != rows[:n])[:8])
        assert np.all(a[n if written else 0:] == SENT), (what, name)   # behind min(hits, capacity) nothing is touched; NULL: nothing is
    if D:
        got = D.read()
        exp = D.with_rows(want.D[:n])
        assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
    A.unchanged()
    B.unchanged()
    if NA and NB:
        p = dev.near_plan(NA, NB, ncols, (wc0, wc1))
        fams = [family(p, 0), "gf2_near_scan_kernel"]
        selects = capn and ((store and ncols) or any(nm in given for nm in ARRAYS))
        if selects:
            fams.append(family(p, 1))
        assert_route(k0, k1, fams)
        assert selects or not launched(k0, k1, family(p, 1)), what        # the counts only: one pass over the pairs
        assert not launched(k0, k1, "gf2_join_"), what                    # the join's kernels stay where they are
    else:
        assert not launched(k0, k1, "gf2_near_"), what
    return want, n


def run_nearest(dev, L, wa, wb, ncols, wcols, flags=0, given=("idx", "dist"), layouts=(EE, EE), stream=None, same=False):
    """one gf2_nearest_dev call on dirty windows against the yardstick -> (idx, dist) of the yardstick"""
    import torch
    NA, NB = wa.shape[0], wb.shape[0]
    want = nr.nearest(wa, wb, ncols, wcols[0], wcols[1], flags)
    A = View(dev, NA, ncols, layouts[0], 17 * NA + wcols[0], wa)
    B = A if same else View(dev, NB, ncols, layouts[1], 19 * NB + wcols[1] + 1, wb)
    ints = {name: guarded(max(NA, 1)) for name in ("idx", "dist")}
    args = {name: ints[name][1] if name in given else dev.SKIP for name in ("idx", "dist")}
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.nearest(A.m, B.m, wcols, flags=flags, stream=stream, **args)
    assert out == (None, None)
    torch.cuda.synchronize()
    k1 = census(L)
    what = (NA, NB, ncols, wcols, flags, given, layouts)
    for name, exp in zip(("idx", "dist"), want):
        a = read_guarded(ints[name][0])
        if name in given:
            assert np.array_equal(a[:NA], exp), (what, name, np.flatnonzero(a[:NA] != exp)[:8], a[:8], exp[:8])
        assert np.all(a[NA if name in given else 0:] == SENT), (what, name)
    A.unchanged()
    B.unchanged()
    if NA and NB:
        assert_route(k0, k1, [family(dev.near_plan(NA, NB, ncols, wcols), 2), "gf2_near_fold_kernel"])
    else:
        assert not launched(k0, k1, "gf2_near_"), what
    return want


# ---- row counts --------------------------------------------------------------------------------------------------------------------

SIZES = [(0, 5), (5, 0), (1, 1), (1, 600), (600, 1), (63, 600), (64, 64), (65, 255), (255, 65), (256, 257), (257, 256), (600, 63), (600, 600),
         (0, 0)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_row_counts(dev, L, size):
    NA, NB = size
    ncols, wcols = 128, (3, 100)                             # the range crosses a word boundary
    wa, wb = g.random_words(NA, ncols, 900 + NA), g.random_words(NB, ncols, 901 + NB)
    win = median_window(wa, wb, ncols, wcols)
    want, _ = run_pairs(dev, L, wa, wb, ncols, wcols, win, layouts=(OE, EE, EO))
    if NA * NB > 20:
        assert 0.3 * NA * NB <= want.hits <= 0.8 * NA * NB        # about half the pairs
    else:
        assert want.hits <= NA * NB
    run_pairs(dev, L, wa, wb, ncols, wcols, win, cap="equal", layouts=(EE, OO, OE), given=("ib", "wt"), want=want)
    run_nearest(dev, L, wa, wb, ncols, wcols, layouts=(EO, OE))


# ---- every kernel instance ---------------------------------------------------------------------------------------------------------

WIDTHS = [1, 37, 64, 65, 128, 256, 300, 1024, 1025, 1100]


def test_the_widths_cover_the_kernels(dev):
    kernels = [dev.near_plan(257, 300, n)[0] for n in WIDTHS]
    assert kernels == [1, 1, 1, 2, 2, 4, 8, 16, 0, 0]          # the last two take the wide path


@pytest.mark.parametrize("ncols", WIDTHS)
def test_widths_and_alignment(dev, L, ncols):
    """the whole row as the range: every kernel instance, counting, selecting and ranking; the last word of a row is partial and dirty
    wherever ncols is no multiple of 64"""
    NA, NB = 257, 300
    layouts = LAYOUTS[WIDTHS.index(ncols) % len(LAYOUTS)]
    wa, wb = g.random_words(NA, ncols, ncols), g.random_words(NB, ncols, ncols + 1)
    if ncols > 8:
        wb[NB - 3] = wa[2]           # a repeated row: a zero row, a hit of every window from 0, and the nearest row of row 2
        wb[7] = wa[2]
    wcols = (0, ncols)
    win = median_window(wa, wb, ncols, wcols)
    want, n = run_pairs(dev, L, wa, wb, ncols, wcols, win, layouts=layouts)
    assert 0 < want.hits and n == want.hits
    if ncols > 8:
        t = list(zip(want.ia, want.ib)).index((2, NB - 3))
        assert not want.D[t].any() and want.wt[t] == 0 and want.hits < NA * NB
    run_pairs(dev, L, wa, wb, ncols, wcols, (win[1] + 1, ncols), cap="less", layouts=layouts, given=("ia", "wt"))     # the other half
    idx, dist = run_nearest(dev, L, wa, wb, ncols, wcols, layouts=layouts[:2])
    if ncols > 8:
        assert (idx[2], dist[2]) == (7, 0)                   # the lower of the two repeated rows


# ---- ranges and windows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wcols", [(70, 100), (60, 140), (0, 200), (3, 193), (129, 200), (191, 200), (0, 0), (77, 77), (200, 200)],
                         ids=lambda w: "%d-%d" % w)
def test_weight_ranges(dev, L, wcols):
    """inside one word, across a word boundary, the whole row, ending on the last partial word (whose excess bits are dirty), empty"""
    ncols = 200
    wa, wb = g.random_words(300, ncols, 77), g.random_words(200, ncols, 78)
    wb[9] = wa[4]
    if wcols[0] == wcols[1]:
        for wlo in (0, 1):                                    # an empty range weighs 0
            want, n = run_pairs(dev, L, wa, wb, ncols, wcols, (wlo, wlo + 3), layouts=(EE, OE, OO))
            assert want.hits == n == (300 * 200 if wlo == 0 else 0) and not want.wt.any()
        idx, dist = run_nearest(dev, L, wa, wb, ncols, wcols, layouts=(OO, EE))
        assert not idx.any() and not dist.any()               # every row is at distance 0: the lowest one
        return
    win = median_window(wa, wb, ncols, wcols)
    want, _ = run_pairs(dev, L, wa, wb, ncols, wcols, win, layouts=(EO, OE, EE))
    bits = g.words_to_bits(want.D, ncols)
    assert 0 < want.hits < 300 * 200 and np.array_equal(want.wt, bits[:, wcols[0]:wcols[1]].sum(axis=1)) and want.wt.max() <= win[1]
    idx, dist = run_nearest(dev, L, wa, wb, ncols, wcols, layouts=(OE, EO))
    assert (idx[4], dist[4]) == (9, 0)


def test_windows_of_weights(dev, L):
    """no hit, every pair a hit, a few hits, wlo > 0, whi past the width"""
    ncols, wcols = 200, (100, 170)
    wa, wb = g.random_words(300, ncols, 79), g.random_words(200, ncols, 80)
    wb[7] = wa[5]
    d = nr.distances(wa, wb, ncols, *wcols).reshape(-1)
    k = int(np.median(d))
    few = int(np.sort(d)[12])
    width = wcols[1] - wcols[0]
    for win in ((0, 0), (k, k), (0, width), (0, width + 1000), (k + 1, (1 << 31) - 1), (width, width), (width + 1, width + 5), (1, few), (0, few),
                (1, 1)):
        want, _ = run_pairs(dev, L, wa, wb, ncols, wcols, win, layouts=(EO, OE, EE))
        assert want.hits == int(((d >= win[0]) & (d <= win[1])).sum())
        if win[0] == 0 and win[1] >= width:
            assert want.hits == 300 * 200
    assert (d == 0).sum() == 1 and (d > width).sum() == 0 and 12 <= ((d >= 1) & (d <= few)).sum() < 200 and not (d == 1).any()


# ---- capacity, the index-only mode -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def capacity_case():
    ncols, wcols = 257, (10, 250)
    wa, wb = g.random_words(500, ncols, 55), g.random_words(400, ncols, 56)
    few = int(np.sort(nr.distances(wa, wb, ncols, *wcols).reshape(-1))[2000])
    return wa, wb, ncols, wcols, (0, few), nr.near_pairs(wa, wb, ncols, wcols[0], wcols[1], 0, few)


SUBSETS = [tuple(s) for r in range(4) for s in itertools.combinations(ARRAYS, r)]


@pytest.mark.parametrize("store", [True, False], ids=["rows", "no-rows"])
@pytest.mark.parametrize("cap", ["zero", 1, "hits-1", "equal", "more"])
def test_capacity(dev, L, cap, store):
    """a capacity below, equal to and above the hits; D with and without data; each of ia, ib and wt given or NULL"""
    wa, wb, ncols, wcols, win, want = capacity_case()
    assert 2000 <= want.hits < 3000
    capn = want.hits - 1 if cap == "hits-1" else cap
    for given in SUBSETS if cap in ("hits-1", "more") else (ARRAYS, ()):
        _, n = run_pairs(dev, L, wa, wb, ncols, wcols, win, cap=capn, given=given, store=store, layouts=(OO, EE, OE), want=want)
        assert n == min(want.hits, capacity(capn, want.hits))


# ---- the flags ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same", [True, False], ids=["A-is-B", "A-and-B"])
@pytest.mark.parametrize("flags", [OFF, UPPER, OFF | UPPER])
def test_flags(dev, L, flags, same):
    """600 rows: two blocks of rows of A, the diagonal crosses both"""
    N, ncols, wcols = 600, 100, (0, 100)
    wa = g.random_words(N, ncols, 14)
    wa[300] = wa[4]
    wa[599] = wa[513]
    wb = wa if same else g.random_words(N - 37, ncols, 15)        # the flags compare row numbers alone: another pool, another height
    win = median_window(wa, wb, ncols, wcols, flags)
    want, _ = run_pairs(dev, L, wa, wb, ncols, wcols, win, flags=flags, same=same, layouts=(OO, OO, EE))
    pairs_ = set(zip(want.ia.tolist(), want.ib.tolist()))
    assert want.hits > 1000 and all((i < j) if flags & UPPER else (i != j) for i, j in pairs_)
    if same:
        assert ((4, 300) in pairs_) and ((300, 4) in pairs_) == (not flags & UPPER)
    idx, dist = run_nearest(dev, L, wa, wb, ncols, wcols, flags=flags, same=same, layouts=(EE, EE))
    if same:
        assert (idx[4], dist[4]) == (300, 0) and (idx[513], dist[513]) == (599, 0)
        assert (idx[599], dist[599]) == ((-1, -1) if flags & UPPER else (513, 0))
    # near duplicates of a pool, every unordered pair once
    want, n = run_pairs(dev, L, wa, wb, ncols, wcols, (0, 0), flags=flags, same=same, cap=5)
    if same:
        assert list(zip(want.ia, want.ib)) == ([(4, 300), (513, 599)] if flags & UPPER else [(4, 300), (300, 4), (513, 599), (599, 513)])


def test_flags_skip_and_keep_whole_tiles(dev, L):
    """1300 rows of 1024 columns: three blocks of rows of A, eleven chunks of one tile each.  Under GF2_NEAR_UPPER a workgroup finds tiles
    whose pairs are all excluded, all admitted, and both"""
    N, ncols = 1300, 1024
    p = dev.near_plan(N, N, ncols)
    assert p[0] == 16 and p[3] >= 10 and 2 * p[4] < p[2] and 3 * p[2] > N > 2 * p[2]
    wa = g.random_words(N, ncols, 16)
    for i, j in ((3, 1299), (511, 512), (512, 511), (700, 700 + p[4]), (1290, 5)):
        wa[j, :8] = wa[i, :8]                                 # pairs that are near on the first 512 columns
    for flags in (UPPER, OFF):
        want, _ = run_pairs(dev, L, wa, wa, ncols, (0, 512), (0, 180), flags=flags, same=True)
        assert 3 <= want.hits <= 40
        run_nearest(dev, L, wa, wa, ncols, (0, ncols), flags=flags, same=True)


# ---- nearest -----------------------------------------------------------------------------------------------------------------------

def test_nearest_with_planted_ties(dev, L):
    ncols, wcols = 256, (0, 256)
    wa, wb = g.random_words(70, ncols, 21), g.random_words(900, ncols, 22)
    for j in (850, 400, 77):                                   # duplicate rows of B: the lowest one wins
        wb[j] = wb[33]
    wa[9] = wb[33]
    wa[10] = wb[33]
    wa[10, 0] ^= np.uint64(1)
    idx, dist = run_nearest(dev, L, wa, wb, ncols, wcols, layouts=(OO, EO))
    assert (idx[9], dist[9]) == (33, 0) and (idx[10], dist[10]) == (33, 1)
    for given in (("idx",), ("dist",)):
        run_nearest(dev, L, wa, wb, ncols, wcols, given=given)
    same = np.tile(g.random_words(1, ncols, 23), (130, 1))     # all rows equal
    idx, dist = run_nearest(dev, L, same, same, ncols, wcols, same=True)
    assert not idx.any() and not dist.any()
    idx, dist = run_nearest(dev, L, same, same, ncols, wcols, flags=OFF, same=True)
    assert idx.tolist() == [1] + [0] * 129 and not dist.any()
    idx, dist = run_nearest(dev, L, same, same, ncols, wcols, flags=UPPER, same=True)
    assert idx.tolist() == list(range(1, 130)) + [-1] and dist.tolist() == [0] * 129 + [-1]
    idx, dist = run_nearest(dev, L, wa, wb[:1], ncols, wcols, flags=OFF)               # a B of one row: row 0 of A has no partner
    assert (idx[0], dist[0]) == (-1, -1) and not idx[1:].any() and (dist[1:] > 0).all()
    idx, dist = run_nearest(dev, L, wa, wb[:0], ncols, wcols)                           # an empty B
    assert (idx == -1).all() and (dist == -1).all()


# ---- shapes where the plan cuts B into chunks ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chunked_case(NA, NB, ncols):
    from m4ri_rust_amd import device
    p = device.near_plan(NA, NB, ncols)
    rows, S, chunk = p[2], p[3], p[4]
    wa, wb = g.random_words(NA, ncols, NA), g.random_words(NB, ncols, NB)
    last_a = min(rows, NA) - 1
    plant = [(0, 0), (0, chunk - 1), (0, chunk), (last_a, 2 * chunk - 1), (last_a, 2 * chunk), (NA - 1, NB - 1), (NA - 1, (S - 1) * chunk),
             (2, chunk + 5), (2, chunk + 9), (2, chunk + 70)]             # the last three: one cell with three hits
    if NA > rows:
        plant += [(rows, 3 * chunk - 1), (rows, 3 * chunk), (rows - 1, 4 * chunk - 1), (rows, 4 * chunk)]
    for t, (i, j) in enumerate(plant):
        wb[j] = wa[i]
        wb[j, 0] ^= np.uint64(1 << (t % 3))                                # distance 1; every row of B is planted once
    assert len({j for _, j in plant}) == len(plant)
    want = nr.near_pairs(wa, wb, ncols, 0, ncols, 0, 1)
    assert set(plant) <= set(zip(want.ia.tolist(), want.ib.tolist())) and want.hits < len(plant) + 4
    return wa, wb, p, plant, want


@pytest.mark.parametrize("shape", [(5, 70000, 64), (700, 20000, 128)], ids=lambda s: "%dx%dx%d" % s)
def test_chunks_of_b(dev, L, shape):
    """NA = 5: one block of rows, many chunks; NA = 700: several blocks and several chunks.  The hits straddle the borders of chunks
    and of blocks, and a capacity ends in the middle of a cell"""
    NA, NB, ncols = shape
    wa, wb, p, plant, want = chunked_case(*shape)
    assert p[3] > 8 and (NA > p[2]) == (NA == 700)
    run_pairs(dev, L, wa, wb, ncols, (0, ncols), (0, 1), want=want, layouts=(EO, OE, EE))
    t = list(zip(want.ia, want.ib)).index((2, p[4] + 9))      # the second hit of a cell of three
    assert (want.ia[t - 1], want.ia[t + 1]) == (2, 2) and want.ib[t - 1] // p[4] == want.ib[t + 1] // p[4] == 1
    for cap in (t, t + 1):
        run_pairs(dev, L, wa, wb, ncols, (0, ncols), (0, 1), cap=cap, want=want, layouts=(EE, EE, OO))
    idx, dist = run_nearest(dev, L, wa, wb, ncols, (0, ncols), layouts=(OO, EE))
    assert dist[0] <= 1 and dist[NA - 1] <= 1


# ---- the join with an empty window, on the device -----------------------------------------------------------------------------------

def test_equal_to_join_select_on_the_device(dev):
    """flags == 0: D and all arrays of gf2_join_select_dev(b = 0)"""
    NA, NB, ncols, wcols = 3000, 2500, 256, (70, 256)
    A, B = dev.DMat.random(NA, ncols, 5), dev.DMat.random(NB, ncols, 6)
    wlo, whi = 0, 70
    S, count, hits, ia, ib, wt = dev.join_select(A, B, 0, 0, wcols, wlo, whi)
    n = int(hits.read(None)[0])
    assert int(count.read(None)[0]) == NA * NB and 50 < n < NA * NB // 100
    D2, hits2, ia2, ib2, wt2 = dev.near_pairs(A, B, wcols, wlo, whi)               # sized by a counts-only call
    assert D2.nrows == n == int(hits2.read(None)[0]) and hits2.read(None).dtype == np.int64
    assert np.array_equal(D2.to_words(), S.to_words())
    for got, exp in zip((ia2, ib2, wt2), (ia, ib, wt)):
        assert np.array_equal(got.read(None), exp.read(None))
    cut = n // 2                                                                    # ... and with a capacity below the hits
    S3, _, _, ia3, ib3, wt3 = dev.join_select(A, B, 0, 0, wcols, wlo, whi, cap=cut)
    D4, hits4, ia4, ib4, wt4 = dev.near_pairs(A, B, wcols, wlo, whi, cap=cut)
    assert int(hits4.read(None)[0]) == n and np.array_equal(D4.to_words(), S3.to_words())
    for got, exp in zip((ia4, ib4, wt4), (ia3, ib3, wt3)):
        assert np.array_equal(got.read(None), exp.read(None))


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------

def test_wrappers_size_their_results(dev):
    NA, NB, ncols, wcols = 3000, 2000, 100, (0, 41)
    wa, wb = g.random_words(NA, ncols, 8), g.random_words(NB, ncols, 9)
    want = nr.near_pairs(wa, wb, ncols, wcols[0], wcols[1], 0, 7)
    assert 0 < want.hits < 20000
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    D, hits, ia, ib, wt = dev.near_pairs(A, B, wcols, 0, 7)                           # neither D nor cap: a counts-only call first
    assert D.nrows == want.hits and np.array_equal(D.to_words(), want.D) and int(hits.read(None)[0]) == want.hits
    assert np.array_equal(ia.read(None), want.ia) and np.array_equal(ib.read(None), want.ib) and np.array_equal(wt.read(None), want.wt)
    D, ia, ib, wt = A.near_pairs(B, wcols, 0, 7)
    assert np.array_equal(D.to_words(), want.D) and np.array_equal(ia.read(None), want.ia) and np.array_equal(wt.read(None), want.wt)
    D, hits, ia, ib, wt = dev.near_pairs(A, B, wcols, 0, 7, cap=10, ia=dev.SKIP)
    assert D.nrows == 10 and ia is None and int(hits.read(None)[0]) == want.hits and np.array_equal(D.to_words(), want.D[:10])
    assert np.array_equal(ib.read(None), want.ib[:10])
    none, hits, ia, ib, wt = dev.near_pairs(A, B, wcols, 0, 7, store=False, wt=dev.SKIP)
    assert none is None and wt is None and np.array_equal(ia.read(None), want.ia) and np.array_equal(ib.read(None), want.ib)
    with pytest.raises(ValueError):
        dev.near_pairs(A, B, wcols, 0, 7, D=D, store=False)
    with pytest.raises(Exception, match="flags"):
        dev.near_pairs(A, B, wcols, 0, 7, flags=4, cap=1)
    E, ia, ib, wt = A.near_pairs(B, wcols, 42, 50)                                    # no hit: an empty matrix
    assert E.nrows == 0 and E.ncols == ncols and ia is None
    # near duplicates inside a pool, and the nearest codeword of a list
    up = A.near_pairs(A, None, 0, 32, flags=dev.NEAR_UPPER)
    ref = nr.near_pairs(wa, wa, ncols, 0, ncols, 0, 32, nr.UPPER)
    assert ref.hits > 20 and up[0].nrows == ref.hits and np.array_equal(up[1].read(None), ref.ia) and np.array_equal(up[2].read(None), ref.ib)
    idx, dist = A.nearest(B)
    ridx, rdist = nr.nearest(wa, wb, ncols, 0, ncols)
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist) and idx.dtype == np.int32
    idx, dist = dev.nearest(A, B, wcols, dist=dev.SKIP)
    assert dist is None and np.array_equal(idx.read(None), nr.nearest(wa, wb, ncols, *wcols)[0])
    with pytest.raises(Exception, match="both null"):
        dev.nearest(A, B, idx=dev.SKIP, dist=dev.SKIP)
    assert np.array_equal(A.to_words(), wa) and np.array_equal(B.to_words(), wb)


def test_two_calls_give_the_same_bits(dev, L):
    NA, NB, ncols, wcols = 1500, 3000, 192, (0, 192)
    wa, wb = g.random_words(NA, ncols, 21), g.random_words(NB, ncols, 22)
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    results = []
    for _ in range(2):
        D, hits, ia, ib, wt = dev.near_pairs(A, B, wcols, 0, 75, cap=5 * NA)
        idx, dist = dev.nearest(A, B, wcols)
        n = int(hits.read(None)[0])
        results.append((n, D.to_words()[:n], ia.read(None)[:n], ib.read(None)[:n], wt.read(None)[:n], idx.read(None), dist.read(None)))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert 0 < results[0][0] <= 5 * NA


# ---- views, dirty scratch, streams -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", dv.LAYOUTS)
def test_strided_offset_views_of_dirty_parents(dev, layout):
    """tests/dev_views.py: at least one dirty row above and two below the window, dirty words left and right of it; WIDE: a column
    range of a wider matrix"""
    import torch
    NA, NB, ncols, wcols = 300, 270, 300, (61, 290)
    A, B = dv.View(dev, NA, ncols, layout, 31), dv.View(dev, NB, ncols, dv.LAYOUTS[(dv.LAYOUTS.index(layout) + 2) % 5], 32)
    wa, wb = A.window(), B.window()
    win = median_window(wa, wb, ncols, wcols)
    want = nr.near_pairs(wa, wb, ncols, wcols[0], wcols[1], 0, win[1] - 12)
    assert 5 < want.hits < NA * NB
    D = dv.View(dev, want.hits + 2, ncols, layout, 33)
    out = dev.near_pairs(A.m, B.m, wcols, 0, win[1] - 12, D=D.m)
    idx, dist = dev.nearest(A.m, B.m, wcols)
    torch.cuda.synchronize()
    rows = D.window().copy()
    rows[:want.hits] = want.D
    assert np.array_equal(D.read(), D.expect(rows)) and int(out[1].read(None)[0]) == want.hits
    assert np.array_equal(out[2].read(None)[:want.hits], want.ia) and np.array_equal(out[3].read(None)[:want.hits], want.ib)
    ridx, rdist = nr.nearest(wa, wb, ncols, *wcols)
    assert np.array_equal(idx.read(None), ridx) and np.array_equal(dist.read(None), rdist)
    A.unchanged("A")
    B.unchanged("B")


def test_on_dirty_scratch(dev, L):
    """the cells come from a cache in which every block holds a pattern, and no block comes fresh from the driver"""
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for NA, NB, ncols, flags in ((1100, 2000, 128, 0), (700, 5000, 320, UPPER), (300, 900, 1100, 0)):
            wa, wb = g.random_words(NA, ncols, NA), g.random_words(NB, ncols, NB)
            wcols = (0, ncols)
            win = median_window(wa[:100], wb[:100], ncols, wcols)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run_pairs(dev, L, wa, wb, ncols, wcols, (0, win[1] - ncols // 12), flags=flags, stream=stream)
            run_nearest(dev, L, wa, wb, ncols, wcols, flags=flags, stream=stream)
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the distance search on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pools are written by gf2_dmat_fill_random on the caller's stream, behind a sleep; the same calls are enqueued twice behind
    it, into two destinations, before anything synchronises.  Both must hold what the yardstick makes of the seeded pools."""
    import torch
    NA, NB, ncols, seed, wcols = 2001, 3003, 200, 0xB1E, (70, 200)
    wa, wb = lr.seeded_words(seed, ncols, np.arange(NA)), lr.seeded_words(seed + 1, ncols, np.arange(NB))
    want = nr.near_pairs(wa, wb, ncols, wcols[0], wcols[1], 0, 45)
    ridx, rdist = nr.nearest(wa, wb, ncols, *wcols)
    n = want.hits
    assert 0 < n < 20000
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ta = torch.full((NA, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    tb = torch.full((NB, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    A, B = dev.DMat.from_torch(ta, ncols), dev.DMat.from_torch(tb, ncols)
    outs = []
    for _ in range(2):
        td = torch.full((n + 2, 4), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.from_torch(td, ncols), guarded(2), guarded(n + 2), guarded(n + 2), guarded(n + 2), guarded(NA), guarded(NA)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    A.fill_random(seed, s)
    B.fill_random(seed + 1, s)
    for td, D, (th, ph), (ti, pi), (tj, pj), (tw, pw), (tx, px), (ty, py) in outs:
        dev.near_pairs(A, B, wcols, 0, 45, D=D, hits=ph, ia=pi, ib=pj, wt=pw, stream=s)
        dev.nearest(A, B, wcols, idx=px, dist=py, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for td, D, (th, ph), (ti, pi), (tj, pj), (tw, pw), (tx, px), (ty, py) in outs:
        rows = td.cpu().numpy().view(np.uint64)
        assert int(read_guarded(th).view(np.int64)[0]) == n
        assert np.array_equal(rows[:n], want.D) and np.all(rows[n:] == np.uint64(0x1111111111111111))
        assert np.array_equal(read_guarded(ti)[:n], want.ia) and np.array_equal(read_guarded(tj)[:n], want.ib)
        assert np.array_equal(read_guarded(tw)[:n], want.wt)
        assert np.array_equal(read_guarded(tx), ridx) and np.array_equal(read_guarded(ty), rdist)


# ---- past 2^32 ---------------------------------------------------------------------------------------------------------------------

def test_hits_of_exactly_2_to_32(dev, L):
    """65 536 rows a side, 64 columns, every distance is at most 64: all 2^32 pairs are hits.  Counts only"""
    import torch
    N, ncols = 65536, 64
    A, B = dev.DMat.random(N, ncols, 41), dev.DMat.random(N, ncols, 42)
    th, ph = guarded(2)
    ints = [guarded(1) for _ in ARRAYS]
    torch.cuda.synchronize()
    dev.near_pairs(A, B, (0, ncols), 0, 64, D=dev.DMat.wrap(None, 0, ncols, 2), hits=ph, ia=ints[0][1], ib=ints[1][1], wt=ints[2][1])
    torch.cuda.synchronize()
    assert int(read_guarded(th).view(np.int64)[0]) == 1 << 32
    for t, _ in ints:
        assert np.all(read_guarded(t) == SENT)
    th, ph = guarded(2)
    dev.near_pairs(A, A, (0, ncols), 0, 64, flags=UPPER, D=dev.DMat.wrap(None, 0, ncols, 2), hits=ph, ia=dev.SKIP, ib=dev.SKIP, wt=dev.SKIP)
    torch.cuda.synchronize()
    assert int(read_guarded(th).view(np.int64)[0]) == N * (N - 1) // 2


def test_a_view_of_a_parent_past_4gib(dev, L):
    """B: 70 000 rows of 128 columns, 8192 words apart: its last rows start behind byte offset 2^32 of the parent.  Only the view's
    words are written (gf2_copy_block_dev from a compact upload); A (256 rows) and D are compact"""
    import torch
    NA, NB, ncols, ld, wcols = 256, 70000, 128, 8192, (0, 128)
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((NB, ld), dtype=torch.int64, device="cuda")
    assert NB * ld * 8 > lr.LIMIT_BYTES
    wa, wb = g.random_words(NA, ncols, 70), g.random_words(NB, ncols, 71)
    r_hi = lr.straddle(ld, NB)[1]
    wb[NB - 1] = wa[5]                            # pairs whose row of B lies behind 2^32
    wb[NB - 2] = wa[200] ^ np.uint64(3)
    B = dev.DMat.wrap(t.data_ptr() + 8 * 6, NB, ncols, ld, keep=t)
    dev.copy_block(B, 0, 0, dev.DMat.from_words(wb, ncols), 0, 0, NB, ncols)
    A = dev.DMat.from_words(wa, ncols)
    want = nr.near_pairs(wa, wb, ncols, wcols[0], wcols[1], 0, 40)
    D, hits, ia, ib, wt = dev.near_pairs(A, B, wcols, 0, 40, cap=want.hits + 1)
    assert int(hits.read(None)[0]) == want.hits and 2 < want.hits < 5000
    assert np.array_equal(ia.read(None)[:-1], want.ia) and np.array_equal(ib.read(None)[:-1], want.ib)
    assert np.array_equal(wt.read(None)[:-1], want.wt) and np.array_equal(D.to_words()[:-1], want.D)
    assert (want.ib > r_hi).sum() >= 2 and not want.D[list(zip(want.ia, want.ib)).index((5, NB - 1))].any()
    idx, dist = dev.nearest(A, B, wcols)
    ridx, rdist = nr.nearest(wa, wb, ncols, *wcols)
    assert np.array_equal(idx.read(None), ridx) and np.array_equal(dist.read(None), rdist) and (ridx[5], ridx[200]) == (NB - 1, NB - 2)
    del t, B, D
    gc.collect()
    torch.cuda.empty_cache()
