"""GPU tests of include/m4ri_hip_join_select.h: gf2_join_select_dev bit for bit against the numpy yardstick of tests/join_select_ref.py
(the join of tests/join_ref.py and a filter; itself checked against the definition by tests/test_join_select_reference.py): the rows of
D that are written, the rest of D, the words around D, `count`, `hits`, and `ia`, `ib` and `wt` up to min(hits, capacity).

The harness is that of tests/test_gpu_join.py: every operand is a window of a dirty parent (View of tests/test_gpu_lf1.py) and the whole
parent of D is compared afterwards; the int outputs lie between sentinels and hold a pattern before the call; A and B are unchanged
afterwards; the launch census is checked per call.

R (sorted positions of A per run), G (outputs per round of the scatter) and the lanes of the two kernels are read from
gf2_join_select_plan, never written down here; which kernels ran is read from the launch census."""
import gc
import itertools

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import join_ref as jr
import join_select_ref as js
import limits_ref as lr
from census_util import assert_route, census
from lf2_ref import keys
from test_gpu_join import LAYOUT_TRIPLES, WINDOWS, count_of, drawn, keyed, pools, sort_families, stern_pools
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded

pytestmark = pytest.mark.gpu

ARRAYS = ("ia", "ib", "wt")


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


def plan_of(ncols=128):
    """(R, G of rows of ncols columns)"""
    try:
        from m4ri_rust_amd import device
        p = device.join_select_plan(1000, 1000, ncols, 8)
        return p[2], p[8]
    except Exception:   # not built yet: the fixture builds; test_the_cases_are_the_plans checks the sizes
        return 1024, 256


R, G = plan_of()


def test_the_cases_are_the_plans(dev):
    p = dev.join_select_plan(5, 7, 128, 30)
    assert (R, G) == plan_of() == (p[2], p[8]) and R >= 256 and 2 <= G <= p[1] and R % G == 0
    assert R == dev.join_plan(5, 7, 128, 30)[2]
    assert [dev.join_select_plan(10, 20, 64, b)[0] for b in (0, 1, 8, 9, 16, 17, 30)] == [0, 1, 1, 2, 2, 3, 4]


def capacity(cap, hits):
    return {"zero": 0, "less": hits // 2, "equal": hits, "more": hits + 7}[cap] if isinstance(cap, str) else cap


def median_window(wa, wb, ncols, c0, b, wcols):
    """a window that about half the pairs meet: from 0 to the median weight"""
    wt = jr.join(wa, wb, ncols, c0, b, wcols[0], wcols[1]).wt
    return (0, int(np.median(wt))) if len(wt) else (0, 0)


def launched(before, after, family):
    return any(family in k and v > before.get(k, 0) for k, v in after.items())


def run(dev, L, wa, wb, ncols, c0, b, wcols, win, cap="more", given=ARRAYS, store=True, layouts=(EE, EE, EE), stream=None, same=False):
    """one gf2_join_select_dev call on dirty windows against the yardstick -> (the yardstick's result, the hits that were written).
    store=False: D comes without data.  same: B is the view that A is"""
    import torch
    NA, NB = wa.shape[0], wb.shape[0]
    (wc0, wc1), (wlo, whi) = wcols, win
    want = js.select(wa, wb, ncols, c0, b, wc0, wc1, wlo, whi)
    assert want.count == jr.pair_count(keys(wa, c0, b), keys(wb, c0, b)) and want.hits == len(want.ia)
    capn = capacity(cap, want.hits)
    n = min(want.hits, capn)
    A = View(dev, NA, ncols, layouts[0], 11 * NA + c0, wa)
    B = A if same else View(dev, NB, ncols, layouts[1], 7 * NB + b + 1, wb)
    D = View(dev, capn, ncols, layouts[2], 13 * NA + b) if capn and store else None
    Dm = D.m if D else dev.DMat.wrap(None, capn, ncols, max(g.width(ncols), 1))
    (tc, pc), (th, ph) = guarded(2), guarded(2)
    ints = {name: guarded(max(capn, 1)) for name in ARRAYS}
    args = {name: ints[name][1] if name in given and capn else dev.SKIP for name in ARRAYS}
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.join_select(A.m, B.m, c0, b, (wc0, wc1), wlo, whi, D=Dm if store or not capn else None, cap=capn, store=store or not capn,
                          count=pc, hits=ph, stream=stream, **args)
    assert out[0] is (Dm if store or not capn else None) and out[1:] == (None,) * 5
    torch.cuda.synchronize()
    k1 = census(L)
    what = (NA, NB, ncols, c0, b, (wc0, wc1), (wlo, whi), cap, given, store, layouts)
    assert (count_of(tc), count_of(th)) == (want.count, want.hits), what
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
        p = dev.join_select_plan(NA, NB, ncols, b, (wc0, wc1))
        fams = sort_families(b) + ["gf2_join_count_kernel", "gf2_join_scan_kernel", "gf2_join_weigh_kernelILi%dE" % p[3]]
        scatters = capn and ((store and ncols) or any(nm in given for nm in ARRAYS))
        if scatters:
            fams.append("gf2_join_select_scatter_kernelILi%dE" % p[4])
        assert_route(k0, k1, fams)
        assert scatters or not launched(k0, k1, "gf2_join_select_scatter_kernel"), what     # the counts only: one pass over the pairs
        assert not launched(k0, k1, "gf2_join_scatter_kernel"), what                        # no pair leaves the kernel but a hit
    else:
        assert not launched(k0, k1, "gf2_join_"), what
    return want, n


# ---- row counts --------------------------------------------------------------------------------------------------------------------

SIZES = [("0", 0), ("1", 1), ("2", 2), ("63", 63), ("64", 64), ("65", 65), ("R-1", R - 1), ("R", R), ("R+1", R + 1), ("2R+5", 2 * R + 5)]


@pytest.mark.parametrize("nb", ["same", "300"])
@pytest.mark.parametrize("case", SIZES, ids=lambda c: c[0])
def test_row_counts(dev, L, case, nb):
    NA = case[1]
    NB = NA if nb == "same" else 300
    ncols, c0, b, wcols = 128, 60, 9, (3, 100)              # two passes; the window crosses a word boundary
    wa, wb = pools(NA, NB, ncols, c0, b, max(NA // 3, 4), 900 + NA)
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want, _ = run(dev, L, wa, wb, ncols, c0, b, wcols, win, layouts=(OE, EE, EO))
    if NA == 0 or NB == 0:
        assert (want.count, want.hits) == (0, 0)
    elif want.count > 20:
        assert 0.3 * want.count <= want.hits <= 0.8 * want.count      # about half the pairs
    run(dev, L, wb, wa, ncols, c0, b, wcols, win, cap="equal", layouts=(EE, OO, OE), given=("ib", "wt"))     # the sides exchanged


# ---- planted hit patterns ----------------------------------------------------------------------------------------------------------

P_NCOLS, P_C0, P_B, P_WCOLS, FLAG_A, FLAG_B = 128, 3, 9, (64, 128), 70, 100


def planted(NA, NB, fa, fb, seed):
    """all keys equal: output j pairs row j // NB of A with row j % NB of B.  Both pools are zero on the weight range but for one
    flag column each: the pair (i, k) weighs fa[i] + fb[k]"""
    wa, wb = keyed(NA, P_NCOLS, P_C0, P_B, np.full(NA, 0x155), seed), keyed(NB, P_NCOLS, P_C0, P_B, np.full(NB, 0x155), seed + 1)
    wa[:, 1] = np.asarray(fa, dtype=np.uint64) << np.uint64(FLAG_A - 64)
    wb[:, 1] = np.asarray(fb, dtype=np.uint64) << np.uint64(FLAG_B - 64)
    return wa, wb


def test_planted_patterns_the_row_of_b_decides(dev, L):
    """NA = 3, NB = 700: the three rows of A are flagged, so a pair weighs 2 where its row of B is flagged and 1 elsewhere; the rounds of
    the second and third row of A begin at other lanes than those of the first (700 is no multiple of 64)"""
    NA, NB = 3, 700
    assert NB % 64 and NB > 2 * G and NA * NB < R * 1000
    k = np.arange(NB)
    patterns = {"none": k < 0, "all": k >= 0, "first of a round": k % G == 0, "last of a round": k % G == G - 1, "every 64th": k % 64 == 0,
                "every 65th": k % 65 == 0, "the last output": k == NB - 1, "the first wave": k < 64, "all but one": k != 321}
    for name, fb in patterns.items():
        wa, wb = planted(NA, NB, np.ones(NA, dtype=int), fb, 40)
        want, n = run(dev, L, wa, wb, P_NCOLS, P_C0, P_B, P_WCOLS, (2, 2), layouts=(EO, EE, OE))
        assert want.count == NA * NB and want.hits == n == NA * int(fb.sum()), name
        if fb.any():
            assert np.array_equal(want.ib[:int(fb.sum())], np.flatnonzero(fb))
        if name in ("every 64th", "all"):
            run(dev, L, wa, wb, P_NCOLS, P_C0, P_B, P_WCOLS, (1, 1), cap=G + 3)        # the complement, cut inside the second round


def test_planted_patterns_across_runs(dev, L):
    """NA = R + 1 and 2 R + 5 with NB = 5: a run of A has 5 R outputs, the hits straddle rounds, waves and runs"""
    NB = 5
    every = np.ones(NB, dtype=int)
    for NA in (R + 1, 2 * R + 5):
        i = np.arange(NA)
        cases = {
            "no hit": (i < 0, every, "more"),
            "every pair": (i >= 0, every, "more"),
            "one hit, in the last run": (i == NA - 1, np.arange(NB) == 3, "more"),
            "the last run alone": (i >= (NA - 1) // R * R, every, "more"),
            "hits only behind the capacity": (i >= 0, every, 5 * R - 2),          # the capacity ends inside the first run: the others write nothing
            "the capacity is the first run's": (i >= 0, every, 5 * R),
            "a run with hits between two without": ((i >= R) & (i < 2 * R), np.arange(NB) % 2 == 0, "more"),
            "every 13th row of A": (i % 13 == 0, np.arange(NB) != 1, "less"),
        }
        for name, (fa, fb, cap) in cases.items():
            if "between" in name and NA < 2 * R:
                continue
            wa, wb = planted(NA, NB, fa, fb, 50)
            want, n = run(dev, L, wa, wb, P_NCOLS, P_C0, P_B, P_WCOLS, (2, 2), cap=cap, layouts=(EE, OO, EE))
            assert want.count == NA * NB and want.hits == int(np.sum(fa)) * int(np.sum(fb)), name
            assert n == min(want.hits, capacity(cap, want.hits))


# ---- every kernel instance ---------------------------------------------------------------------------------------------------------

# (ncols, weight range): the words of the range give the lanes of the weigh pass, the words of the row those of the row store
SHAPES = [(64, (0, 64)), (100, (10, 90)), (130, (0, 130)), (256, (70, 130)), (256, (0, 256)), (1030, (5, 1000)), (1030, (700, 710)),
          (4160, (4100, 4130)), (4160, (100, 300)), (4160, (64, 4160)), (4160, (0, 4160))]


def test_the_shapes_cover_the_lanes(dev):
    seen = {tuple(dev.join_select_plan(100, 100, n, 4, w)[3:5]) for n, w in SHAPES}
    assert {s[0] for s in seen} == {s[1] for s in seen} == {1, 2, 8, 64}
    assert {(1, 64), (64, 64), (1, 1), (2, 2), (8, 8), (2, 64), (1, 8)} <= seen        # a wide row with a range inside one word among them
    words = lambda w: (w[1] - 1) // 64 - w[0] // 64 + 1   # noqa: E731
    assert {1, 2, 3, 4} <= {words(w) for _, w in SHAPES} and any(4 < words(w) <= 64 for _, w in SHAPES) and any(words(w) > 64 for _, w in SHAPES)


@pytest.mark.parametrize("layouts", LAYOUT_TRIPLES, ids=lambda t: "A%d%d-B%d%d-D%d%d" % (t[0] + t[1] + t[2]))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-w%d-%d" % (s[0], s[1][0], s[1][1]))
def test_widths_ranges_and_alignment(dev, L, shape, layouts):
    ncols, wcols = shape
    b = 5
    c0 = ncols - b               # the window ends with the row
    NA, NB = R + 77, 150         # two runs
    wa, wb = pools(NA, NB, ncols, c0, b, 20, ncols)
    wb[NB - 3] = wa[2]           # a repeated row: a zero row, a hit of every window from 0
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want, n = run(dev, L, wa, wb, ncols, c0, b, wcols, win, layouts=layouts)
    t = list(zip(want.ia, want.ib)).index((2, NB - 3))
    assert not want.D[t].any() and want.wt[t] == 0 and 0 < want.hits < want.count
    run(dev, L, wa, wb, ncols, c0, b, wcols, (win[1] + 1, ncols), cap="less", layouts=layouts, given=("ia", "wt"))     # the other half


# ---- capacity, the index-only mode -------------------------------------------------------------------------------------------------

def capacity_pools():
    ncols, c0, b = 257, 250, 4
    return g.random_words(500, ncols, 55), g.random_words(400, ncols, 56), ncols, c0, b


SUBSETS = [tuple(s) for r in range(4) for s in itertools.combinations(ARRAYS, r)]


@pytest.mark.parametrize("store", [True, False], ids=["rows", "no-rows"])
@pytest.mark.parametrize("given", SUBSETS, ids=lambda s: "+".join(s) or "none")
@pytest.mark.parametrize("cap", ["zero", 1, "hits-1", "equal", "more", "in a round"])
def test_capacity(dev, L, cap, given, store):
    wa, wb, ncols, c0, b = capacity_pools()
    wcols = (10, 250)
    win = median_window(wa, wb, ncols, c0, b, wcols)
    Gn = dev.join_select_plan(500, 400, ncols, b, wcols)[8]
    hits = js.select(wa, wb, ncols, c0, b, wcols[0], wcols[1], win[0], win[1]).hits
    capn = {"hits-1": hits - 1, "in a round": Gn + Gn // 4 + 1}.get(cap, cap)     # the second round of the first run writes a part of its hits
    want, n = run(dev, L, wa, wb, ncols, c0, b, wcols, win, cap=capn, given=given, store=store, layouts=(OO, EE, OE))
    assert want.count > 5000 and want.hits == hits > 2000
    if cap == "in a round":
        assert len(wa) <= R and want.hits > 2 * Gn > n > Gn   # one run; more hits than a round has outputs, fewer than two rounds have


# ---- windows and ranges ------------------------------------------------------------------------------------------------------------

def test_windows_of_weights(dev, L):
    ncols, c0, b, wcols = 200, 90, 6, (100, 170)
    wa, wb = pools(300, 200, ncols, c0, b, 30, 77)
    wb[7] = wa[5]
    wt = jr.join(wa, wb, ncols, c0, b, *wcols).wt
    k = int(np.median(wt))
    width = wcols[1] - wcols[0]
    for win in ((0, 0), (k, k), (0, width), (0, width + 1000), (k + 1, (1 << 31) - 1), (width, width), (width + 1, width + 5), (1, k - 1)):
        want, _ = run(dev, L, wa, wb, ncols, c0, b, wcols, win, layouts=(EO, OE, EE))
        assert want.hits == int(((wt >= win[0]) & (wt <= win[1])).sum())
        if win[0] == 0 and win[1] >= width:
            assert want.hits == want.count > 500
    assert (wt == 0).sum() >= 1 and (wt == k).sum() >= 1 and (wt > width).sum() == 0


@pytest.mark.parametrize("wlo", [0, 1])
@pytest.mark.parametrize("wcols", [(0, 0), (77, 77), (200, 200)], ids=lambda w: "%d-%d" % w)
def test_an_empty_range_weighs_nothing(dev, L, wcols, wlo):
    ncols, c0, b = 200, 90, 6
    wa, wb = pools(300, 200, ncols, c0, b, 30, 77)
    want, n = run(dev, L, wa, wb, ncols, c0, b, wcols, (wlo, wlo + 3), layouts=(EE, OE, OO))
    assert want.count > 500 and want.hits == n == (want.count if wlo == 0 else 0) and not want.wt.any()


@pytest.mark.parametrize("wcols", [(0, 200), (70, 100), (60, 140), (3, 193), (129, 200), (191, 200)], ids=lambda w: "%d-%d" % w)
def test_weight_ranges(dev, L, wcols):
    """the whole row, inside one word, across three words, ending at ncols with ncols % 64 != 0"""
    ncols, c0, b = 200, 90, 6
    wa, wb = pools(300, 200, ncols, c0, b, 30, 77)
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want, _ = run(dev, L, wa, wb, ncols, c0, b, wcols, win, layouts=(EO, OE, EE))
    bits = g.words_to_bits(want.D, ncols)
    assert 0 < want.hits < want.count and np.array_equal(want.wt, bits[:, wcols[0]:wcols[1]].sum(axis=1)) and want.wt.max() <= win[1]


# ---- joins -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: "%d-c%d-b%d" % c)
def test_key_windows(dev, L, case):
    ncols, c0, b = case
    NA, NB = (150, 130) if b < 8 else (R + 5, 700)
    ka, kb = drawn(NA, NB, b, NA // 3, 100 + c0 + b)
    if b >= 8:
        ka[::7] ^= 1 << (b - 1)                # the highest bit of the key, which only the last pass sees
        kb[::5] ^= 1 << (b - 1)
    wa, wb = keyed(NA, ncols, c0, b, ka, 200 + c0 + b), keyed(NB, ncols, c0, b, kb, 300 + c0 + b)
    wcols = (0, ncols)                          # the range includes the window, whose bits are zero in every pair
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want, _ = run(dev, L, wa, wb, ncols, c0, b, wcols, win, layouts=(OO, EE, OE) if c0 else (EE, OE, EE))
    assert want.count > 100 and 0 < want.hits < want.count and (b == 0 or not keys(want.D, c0, b).any())


def test_no_key_in_common(dev, L):
    NA, NB, ncols, c0, b = R + 9, 500, 130, 64, 12
    rng = np.random.default_rng(3)
    wa, wb = keyed(NA, ncols, c0, b, 2 * rng.integers(0, 2000, NA), 4), keyed(NB, ncols, c0, b, 2 * rng.integers(0, 2000, NB) + 1, 5)
    for cap in (7, "zero"):
        want, n = run(dev, L, wa, wb, ncols, c0, b, (0, 64), (0, 64), cap=cap)
        assert (want.count, want.hits, n) == (0, 0, 0)
    assert run(dev, L, wa, keyed(NB, ncols, c0, b, np.full(NB, 4095), 6), ncols, c0, b, (0, 130), (0, 130), cap=3)[0].count == 0


def test_a_class_of_a_straddles_a_run_boundary(dev, L):
    """R - 20 rows of distinct keys, then a class of 50 that begins in the first run and ends in the second"""
    ncols, c0, b, wcols = 128, 33, 16, (64, 128)
    ka = np.concatenate([np.arange(R - 20), np.full(50, R + 5), np.arange(200) + 2 * R])
    kb = np.concatenate([np.full(3, R + 5), np.arange(0, R, 3), np.full(2, 2 * R + 199), np.full(4, 7)])
    rng = np.random.default_rng(8)
    ka, kb = ka[rng.permutation(len(ka))], kb[rng.permutation(len(kb))]
    wa, wb = keyed(len(ka), ncols, c0, b, ka, 8), keyed(len(kb), ncols, c0, b, kb, 9)
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want, _ = run(dev, L, wa, wb, ncols, c0, b, wcols, win)
    in_class = keys(wa, c0, b)[want.ia] == R + 5
    assert want.count == len(np.arange(0, R - 20, 3)) + 4 + 150 + 2 and 10 < in_class.sum() < 150
    first = int(np.flatnonzero(in_class)[0])
    run(dev, L, wa, wb, ncols, c0, b, wcols, win, cap=first + int(in_class.sum()) // 2)          # cut inside the class


def test_b_much_larger_than_a_with_a_giant_class(dev, L):
    """NB = 40 NA, random keys, and one class of B of 3 S rows: the span of every run leaves LDS"""
    S = dev.join_plan(1000, 1000, 64, 8)[4]
    NA, ncols, c0, b, wcols = 400, 64, 11, 12, (23, 64)
    NB = 40 * NA
    assert NB > 3 * S + 1000
    rng = np.random.default_rng(12)
    ka, kb = rng.integers(0, 1 << b, NA), rng.integers(0, 1 << b, NB)
    kb[rng.permutation(NB)[:3 * S]] = 0x777
    ka[[5, 300]] = 0x777
    wa, wb = keyed(NA, ncols, c0, b, ka, 12), keyed(NB, ncols, c0, b, kb, 13)
    want, _ = run(dev, L, wa, wb, ncols, c0, b, wcols, (0, 17))
    assert want.count >= 2 * 3 * S and 100 < want.hits < want.count // 2


def test_a_self_join(dev, L):
    """A and B are one view: all ordered pairs of a class; the window (0, 0) keeps (i, i), the zero rows, and nothing else"""
    N, ncols, c0, b = R + 40, 130, 100, 9
    wa = keyed(N, ncols, c0, b, drawn(N, N, b, N // 4, 14)[0], 14)
    want, n = run(dev, L, wa, wa, ncols, c0, b, (0, 100), (0, 0), same=True, layouts=(OO, OO, EE))
    sizes = np.unique(keys(wa, c0, b), return_counts=True)[1]
    assert want.count == int((sizes * sizes).sum()) and n == want.hits == N and np.array_equal(want.ia, want.ib) and not want.D.any()
    win = median_window(wa, wa, ncols, c0, b, (0, 100))
    want, _ = run(dev, L, wa, wa, ncols, c0, b, (0, 100), win, same=True, layouts=(EE, EE, OO))
    assert N < want.hits < want.count


# ---- past 2^31 ---------------------------------------------------------------------------------------------------------------------

def test_counts_past_2_to_31(dev, L):
    """50 000 rows of one key on either side: 2 500 000 000 pairs.  The rows are drawn from four patterns per side, so the hits follow
    from the 4 x 4 table of the patterns' weights; the window leaves out the lightest cell alone, and the hits pass 2^31 as well.
    1000 of them are written; the yardstick runs on the first row of A, whose 50 000 pairs come first"""
    import torch
    N, ncols, c0, b, wcols = 50000, 96, 70, 21, (0, 64)
    rng = np.random.default_rng(31)
    pa, pb = keyed(4, ncols, c0, b, np.full(4, 0x12345), 80), keyed(4, ncols, c0, b, np.full(4, 0x12345), 81)
    table = np.array([[int(jr.weights(pa[i:i + 1] ^ pb[k:k + 1], *wcols)[0]) for k in range(4)] for i in range(4)])
    cells = np.sort(table.reshape(-1))
    assert cells[0] < cells[1]                    # one lightest cell
    wlo = int(cells[1])
    whi = 64
    da, db = rng.integers(0, 4, N), rng.integers(0, 4, N)
    wa, wb = pa[da], pb[db]
    na, nb = np.bincount(da, minlength=4).astype(object), np.bincount(db, minlength=4).astype(object)
    hits = int(sum(na[i] * nb[k] for i in range(4) for k in range(4) if wlo <= table[i, k] <= whi))
    assert N * N == 2500000000 > hits > 1 << 31
    first = js.select(wa[:1], wb, ncols, c0, b, wcols[0], wcols[1], wlo, whi, limit=1000)
    assert first.hits >= 1000 and len(first.ia) == 1000
    A, B = View(dev, N, ncols, EE, 1, wa), View(dev, N, ncols, OO, 2, wb)
    for cap in (1000, 0):
        D = View(dev, cap, ncols, OO, 3) if cap else None
        Dm = D.m if D else dev.DMat.wrap(None, 0, ncols, 2)
        (tc, pc), (th, ph) = guarded(2), guarded(2)
        ints = [guarded(max(cap, 1)) for _ in ARRAYS]
        torch.cuda.synchronize()
        dev.join_select(A.m, B.m, c0, b, wcols, wlo, whi, D=Dm, count=pc, hits=ph, **{nm: t[1] if cap else dev.SKIP for nm, t in zip(ARRAYS, ints)})
        torch.cuda.synchronize()
        assert (count_of(tc), count_of(th)) == (N * N, hits), cap
        for (t, _), rows in zip(ints, (first.ia, first.ib, first.wt)):
            a = read_guarded(t)
            assert np.array_equal(a[:cap], rows[:cap]) and np.all(a[cap:] == SENT)
        if D:
            assert np.array_equal(D.read(), D.with_rows(first.D))
    A.unchanged()
    B.unchanged()


# ---- the composed route on the device ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [8, 12])
def test_equal_to_join_select_weights_and_gathers_on_the_device(dev, b):
    """gf2_join_dev with enough capacity, gf2_select_weights_dev on its weights, and the gathers of D, ia, ib and wt by its indices"""
    import torch
    N, ncols, c0, wcols = 3 << b, 256, 101, (131, 256)
    A, B = dev.DMat.random(N, ncols, b), dev.DMat.random(N, ncols, b + 100)
    D, count, ia, ib, wt = dev.join(A, B, c0, b, wcols=wcols)
    n = D.nrows
    assert abs(n - N * N / (1 << b)) <= 6 * np.sqrt(N * N / (1 << b))
    wlo, whi = 0, int(np.sort(wt.read(None))[n // 20])                # about one pair in twenty
    idx, hits = dev.select_weights(wt.ptr, n, wlo, whi)
    assert hits == len(idx) and n // 40 < hits < n // 5
    picked = dev.gather_rows(D, idx)[0].to_words()
    at = torch.from_numpy(idx.astype(np.int64)).cuda()
    ints = [torch.from_numpy(x.read(None)).cuda().index_select(0, at).cpu().numpy() for x in (ia, ib, wt)]
    S, count2, hits2, ia2, ib2, wt2 = dev.join_select(A, B, c0, b, wcols, wlo, whi)            # sized by a counts-only call
    assert S.nrows == hits == int(hits2.read(None)[0]) and int(count2.read(None)[0]) == n
    assert np.array_equal(S.to_words(), picked)
    for got, exp in zip((ia2, ib2, wt2), ints):
        assert np.array_equal(got.read(None), exp)
    # the index-only mode gives the same arrays and no rows
    none, _, hits3, ia3, ib3, wt3 = dev.join_select(A, B, c0, b, wcols, wlo, whi, cap=hits + 5, store=False)
    assert none is None and int(hits3.read(None)[0]) == hits
    for got, exp in zip((ia3, ib3, wt3), ints):
        assert np.array_equal(got.read(None)[:hits], exp)


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------

def test_wrappers_size_their_results(dev):
    NA, NB, ncols, c0, b, wcols = 3000, 2000, 100, 41, 10, (0, 41)
    wa, wb = g.random_words(NA, ncols, 8), g.random_words(NB, ncols, 9)
    want = js.select(wa, wb, ncols, c0, b, wcols[0], wcols[1], 5, 17)
    assert 0 < want.hits < want.count
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    D, count, hits, ia, ib, wt = dev.join_select(A, B, c0, b, wcols, 5, 17)          # neither D nor cap: a counts-only call first
    assert D.nrows == want.hits and np.array_equal(D.to_words(), want.D)
    assert int(count.read(None)[0]) == want.count and int(hits.read(None)[0]) == want.hits and hits.read(None).dtype == np.int64
    assert np.array_equal(ia.read(None), want.ia) and np.array_equal(ib.read(None), want.ib) and np.array_equal(wt.read(None), want.wt)
    D, ia, ib, wt = A.join_select(B, c0, b, wcols, 5, 17)
    assert np.array_equal(D.to_words(), want.D) and np.array_equal(ia.read(None), want.ia) and np.array_equal(wt.read(None), want.wt)
    # a capacity below the hits; arrays that are not wanted; rows that are not stored
    D, count, hits, ia, ib, wt = dev.join_select(A, B, c0, b, wcols, 5, 17, cap=10, ia=dev.SKIP)
    assert D.nrows == 10 and ia is None and int(hits.read(None)[0]) == want.hits and np.array_equal(D.to_words(), want.D[:10])
    assert np.array_equal(ib.read(None), want.ib[:10])
    none, count, hits, ia, ib, wt = dev.join_select(A, B, c0, b, wcols, 5, 17, store=False, wt=dev.SKIP)
    assert none is None and wt is None and np.array_equal(ia.read(None), want.ia) and np.array_equal(ib.read(None), want.ib)
    with pytest.raises(ValueError):
        dev.join_select(A, B, c0, b, wcols, 5, 17, D=D, store=False)
    # no hit: an empty matrix
    E, ia, ib, wt = A.join_select(B, c0, b, wcols, 42, 50)
    assert E.nrows == 0 and E.ncols == ncols and ia is None
    assert np.array_equal(A.to_words(), wa) and np.array_equal(B.to_words(), wb)


def test_two_calls_give_the_same_bits(dev, L):
    NA, NB, ncols, c0, b, wcols = 3 * R + 1, 2 * R + 7, 192, 77, 11, (0, 192)
    wa, wb = g.random_words(NA, ncols, 21), g.random_words(NB, ncols, 22)
    win = median_window(wa, wb, ncols, c0, b, wcols)
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    results = []
    for _ in range(2):
        D, count, hits, ia, ib, wt = dev.join_select(A, B, c0, b, wcols, win[0], win[1], cap=3 * NA)
        n = int(hits.read(None)[0])
        results.append((n, int(count.read(None)[0]), D.to_words()[:n], ia.read(None)[:n], ib.read(None)[:n], wt.read(None)[:n]))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert 0 < results[0][0] < results[0][1] == jr.pair_count(keys(wa, c0, b), keys(wb, c0, b)) <= 3 * NA


# ---- dirty scratch, streams, past 4 GiB --------------------------------------------------------------------------------------------

def test_on_dirty_scratch(dev, L):
    """the sorts' work space, the sorted orders and keys, the run sums and the hit sums come from a cache in which every block holds a
    pattern, and no block comes fresh from the driver"""
    import torch
    S = dev.join_plan(1000, 1000, 64, 8)[4]
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for NA, NB, ncols, b in ((3 * R + 5, 2000, 128, 9), (2 * R + 77, 5 * S + 9, 320, 25), (700, 900, 64, 0)):
            wa, wb = pools(NA, NB, ncols, 33, b, NA // 3, NA)
            wcols = (0, ncols)
            win = median_window(wa, wb, ncols, 33, b, wcols) if b else (0, 20)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run(dev, L, wa, wb, ncols, 33, b, wcols, win, stream=stream, cap=20000 if b == 0 else "more")
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the weight-filtered join on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pools are written by gf2_dmat_fill_random on the caller's stream, behind a sleep; the same call is enqueued twice behind it,
    into two destinations, before anything synchronises.  Both must hold what the yardstick makes of the seeded pools."""
    import torch
    NA, NB, ncols, c0, b, seed, wcols = 9001, 7003, 200, 57, 12, 0xB1D, (70, 200)
    wa, wb = lr.seeded_words(seed, ncols, np.arange(NA)), lr.seeded_words(seed + 1, ncols, np.arange(NB))
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want = js.select(wa, wb, ncols, c0, b, wcols[0], wcols[1], win[0], win[1])
    n = want.hits
    assert 0 < n < want.count
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ta = torch.full((NA, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    tb = torch.full((NB, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    A, B = dev.DMat.from_torch(ta, ncols), dev.DMat.from_torch(tb, ncols)
    outs = []
    for _ in range(2):
        td = torch.full((n + 2, 4), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.from_torch(td, ncols), guarded(2), guarded(2), guarded(n + 2), guarded(n + 2), guarded(n + 2)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    A.fill_random(seed, s)
    B.fill_random(seed + 1, s)
    for td, D, (tc, pc), (th, ph), (ti, pi), (tj, pj), (tw, pw) in outs:
        dev.join_select(A, B, c0, b, wcols, win[0], win[1], D=D, count=pc, hits=ph, ia=pi, ib=pj, wt=pw, stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for td, D, (tc, pc), (th, ph), (ti, pi), (tj, pj), (tw, pw) in outs:
        rows = td.cpu().numpy().view(np.uint64)
        assert (count_of(tc), count_of(th)) == (want.count, n)
        assert np.array_equal(rows[:n], want.D) and np.all(rows[n:] == np.uint64(0x1111111111111111))
        assert np.array_equal(read_guarded(ti)[:n], want.ia) and np.array_equal(read_guarded(tj)[:n], want.ib)
        assert np.array_equal(read_guarded(tw)[:n], want.wt)


def test_a_view_of_a_parent_past_4gib(dev, L):
    """A: 70 000 rows of 128 columns, 8192 words apart: its last rows start behind byte offset 2^32 of the parent.  Only the view's
    words are written (gf2_copy_block_dev from a compact upload); B and D are compact"""
    import torch
    NA, NB, ncols, ld, c0, b, wcols = 70000, 3000, 128, 8192, 60, 15, (64, 128)
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((NA, ld), dtype=torch.int64, device="cuda")
    assert NA * ld * 8 > lr.LIMIT_BYTES
    wa, wb = g.random_words(NA, ncols, 70), g.random_words(NB, ncols, 71)
    r_hi = lr.straddle(ld, NA)[1]
    wb[5] = wa[NA - 1]                            # a pair whose row of A lies behind 2^32: a zero row, a hit
    A = dev.DMat.wrap(t.data_ptr() + 8 * 6, NA, ncols, ld, keep=t)
    dev.copy_block(A, 0, 0, dev.DMat.from_words(wa, ncols), 0, 0, NA, ncols)
    B = dev.DMat.from_words(wb, ncols)
    win = median_window(wa, wb, ncols, c0, b, wcols)
    want = js.select(wa, wb, ncols, c0, b, wcols[0], wcols[1], win[0], win[1])
    D, count, hits, ia, ib, wt = dev.join_select(A, B, c0, b, wcols, win[0], win[1], cap=want.hits + 1)
    assert int(count.read(None)[0]) == want.count and int(hits.read(None)[0]) == want.hits
    assert np.array_equal(ia.read(None)[:-1], want.ia) and np.array_equal(ib.read(None)[:-1], want.ib)
    assert np.array_equal(wt.read(None)[:-1], want.wt) and np.array_equal(D.to_words()[:-1], want.D)
    assert (want.ia > r_hi).sum() > 0 and not want.D[list(zip(want.ia, want.ib)).index((NA - 1, 5))].any()
    del t, A, D
    gc.collect()
    torch.cuda.empty_cache()


# ---- end to end --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_stern_collision_end_to_end(dev, seed):
    """the Stern collision of tests/test_gpu_join.py with p = 1, in ONE call: the join on the columns [0, 8), only the pairs of weight
    up to 5 over [8, 128) leave the kernel, into a D of one row.  The planted pair is the only hit, and it is the hit of the three-call
    chain (join, select_weights, gather_rows)"""
    import torch
    Q, s, i, j, e1, wa, wb = stern_pools(seed)
    want = js.select(wa, wb, 128, 0, 8, 8, 128, 0, 5)
    assert want.hits == 1 and (want.ia[0], want.ib[0]) == (i, j) and np.array_equal(g.words_to_bits(want.D, 128)[0], e1)
    A, B = dev.DMat.from_words(wa, 128), dev.DMat.from_words(wb, 128)
    hit = dev.DMat(1, 128)
    (th, ph), (tc, pc), (ti, pi), (tj, pj), (tw, pw) = guarded(2), guarded(2), guarded(1), guarded(1), guarded(1)
    torch.cuda.synchronize()
    dev.join_select(A, B, 0, 8, (8, 128), 0, 5, D=hit, count=pc, hits=ph, ia=pi, ib=pj, wt=pw)
    # the three calls
    D, count, ia, ib, wt = dev.join(A, B, 0, 8, cap=400, wcols=(8, 128))
    idx, found = dev.select_weights(wt.ptr, want.count, 0, 5)
    chain = dev.gather_rows(D, idx)[0]
    torch.cuda.synchronize()
    assert (count_of(tc), count_of(th)) == (want.count, 1) and found == 1 and int(count.read(None)[0]) == want.count
    assert (int(read_guarded(ti)[0]), int(read_guarded(tj)[0]), int(read_guarded(tw)[0])) == (i, j, 5)
    assert (int(ia.read(None)[idx[0]]), int(ib.read(None)[idx[0]])) == (i, j)
    assert np.array_equal(hit.to_words(), chain.to_words()) and np.array_equal(g.words_to_bits(hit.to_words(), 128)[0], e1)
    assert np.array_equal(A.to_words(), wa) and np.array_equal(B.to_words(), wb)
