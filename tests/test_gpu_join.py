"""GPU tests of include/m4ri_hip_join.h: gf2_join_dev bit for bit against the numpy yardstick of tests/join_ref.py (itself checked against
the definition by tests/test_join_reference.py): the rows of D that are written, the rest of D, the words around D, `count`, and `ia`,
`ib` and `wt` up to min(count, capacity).

Every operand is a window of a dirty parent (View of tests/test_gpu_lf1.py): random bits in every word of the parent -- the rows
before and behind the window, the words left and right of it, the excess bits of the last word of A and B -- and the whole parent of D
is compared afterwards.  The int outputs lie between sentinels and hold a pattern before the call.

R (sorted positions of A per run), S (the keys of B that a workgroup stages in LDS at the most) and the lanes per row are read from
gf2_join_plan, never written down here; which kernels ran is read from the launch census."""
import gc
import itertools

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import join_ref as jr
import limits_ref as lr
from census_util import assert_route, census
from lf2_ref import keys
from test_gpu_lf1 import EE, EO, OE, OO, SENT, View, guarded, read_guarded, set_keys

pytestmark = pytest.mark.gpu

ARRAYS = ("ia", "ib", "wt")
LAYOUT_TRIPLES = [(EE, EE, EE), (EO, OE, OO), (OO, EE, EO), (OE, OO, EE), (EE, EO, OE)]   # (A, B, D): every parity on every side


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
        p = device.join_plan(1000, 1000, 256, 8)
        return p[2], p[4]
    except Exception:   # not built yet: the fixture builds; test_the_cases_are_the_plans checks the sizes
        return 1024, 4096


R, S = plan_of()


def test_the_cases_are_the_plans(dev):
    assert (R, S) == plan_of() == (dev.join_plan(5, 7, 64, 30)[2], dev.join_plan(5, 7, 64, 30)[4]) and R >= 256 and S >= 64
    assert [dev.join_plan(10, 20, 64, b)[0] for b in (0, 1, 8, 9, 16, 17, 30)] == [0, 1, 1, 2, 2, 3, 4]


def keyed(N, ncols, c0, b, k, seed):
    """N random rows whose keys are k"""
    return set_keys(g.random_words(N, ncols, seed), c0, b, k)


def drawn(NA, NB, b, classes, seed):
    """NA and NB keys drawn from the same `classes` random values below 2^b"""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 1 << b, max(classes, 1))
    return values[rng.integers(0, len(values), NA)], values[rng.integers(0, len(values), NB)]


def pools(NA, NB, ncols, c0, b, classes, seed):
    ka, kb = drawn(NA, NB, b, classes, seed)
    return keyed(NA, ncols, c0, b, ka, seed + 1), keyed(NB, ncols, c0, b, kb, seed + 2)


def sort_families(b):
    if b == 0:
        return ["gf2_lf2_iota_kernel"]
    return ["gf2_lf2_sort_count_kernel", "gf2_lf2_scan_sums_kernel", "gf2_lf2_scan_group_kernelIi", "gf2_lf2_scan_apply_kernel",
            "gf2_lf2_sort_scatter_kernel"]


def capacity(cap, count):
    return {"zero": 0, "less": count // 2, "equal": count, "more": count + 7}[cap] if isinstance(cap, str) else cap


def count_of(t):
    return int(read_guarded(t)[:2].copy().view(np.int64)[0])


def run(dev, L, wa, wb, ncols, c0, b, cap="more", given=ARRAYS, wcols=None, layouts=(EE, EE, EE), stream=None, same=False):
    """one gf2_join_dev call on dirty windows against the yardstick -> (count, the yardstick's outputs that were written).  same: B is
    the view that A is"""
    import torch
    NA, NB = wa.shape[0], wb.shape[0]
    wc0, wc1 = (0, ncols) if wcols is None else wcols
    count = jr.pair_count(keys(wa, c0, b), keys(wb, c0, b))
    capn = capacity(cap, count)
    n = min(count, capn)
    want = jr.join(wa, wb, ncols, c0, b, wc0, wc1, limit=n)
    assert want.count == count and len(want.ia) == n
    A = View(dev, NA, ncols, layouts[0], 11 * NA + c0, wa)
    B = A if same else View(dev, NB, ncols, layouts[1], 7 * NB + b + 1, wb)
    D = View(dev, capn, ncols, layouts[2], 13 * NA + b) if capn else None
    Dm = D.m if D else dev.DMat.wrap(None, 0, ncols, g.width(ncols))
    tc, pc = guarded(2)
    ints = {name: guarded(max(capn, 1)) for name in ARRAYS}
    args = {name: ints[name][1] if name in given and capn else dev.SKIP for name in ARRAYS}
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.join(A.m, B.m, c0, b, D=Dm, count=pc, wcols=(wc0, wc1), stream=stream, **args)
    assert out[0] is Dm and out[1:] == (None, None, None, None)
    torch.cuda.synchronize()
    what = (NA, NB, ncols, c0, b, cap, given, (wc0, wc1), layouts)
    assert count_of(tc) == count, what
    for name, rows in (("ia", want.ia), ("ib", want.ib), ("wt", want.wt)):
        a = read_guarded(ints[name][0])
        written = name in given and capn
        if written:
            assert np.array_equal(a[:n], rows), (what, name, np.flatnonzero(a[:n] != rows)[:8])
        assert np.all(a[n if written else 0:] == SENT), (what, name)   # behind min(count, capacity) nothing is touched; NULL: nothing is
    if D:
        got = D.read()
        exp = D.with_rows(want.D)
        assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
    A.unchanged()
    B.unchanged()
    if NA and NB:
        fams = sort_families(b) + ["gf2_join_count_kernel", "gf2_join_scan_kernel"]
        if capn:
            fams.append("gf2_join_scatter_kernelILi%dE" % dev.join_plan(NA, NB, ncols, b)[3])
        assert_route(k0, census(L), fams)
    return count, want


# ---- row counts --------------------------------------------------------------------------------------------------------------------

SIZES = [("0", 0), ("1", 1), ("2", 2), ("63", 63), ("64", 64), ("65", 65), ("R-1", R - 1), ("R", R), ("R+1", R + 1), ("2R+5", 2 * R + 5)]


@pytest.mark.parametrize("nb", ["same", "300"])
@pytest.mark.parametrize("case", SIZES, ids=lambda c: c[0])
def test_row_counts(dev, L, case, nb):
    NA = case[1]
    NB = NA if nb == "same" else 300
    ncols, c0, b = 128, 60, 9               # two passes; the window crosses a word boundary
    wa, wb = pools(NA, NB, ncols, c0, b, max(NA // 3, 4), 900 + NA)
    count, _ = run(dev, L, wa, wb, ncols, c0, b, layouts=(OE, EE, EO), wcols=(3, 100))
    if NA == 0 or NB == 0:
        assert count == 0
    run(dev, L, wb, wa, ncols, c0, b, cap="equal", layouts=(EE, OO, OE), given=("ib", "wt"))     # the sides exchanged


# ---- windows -----------------------------------------------------------------------------------------------------------------------

WINDOWS = [(256, c0, b) for b in (0, 1, 8, 9, 16, 17, 30) for c0 in (0, 37, 50)]
WINDOWS += [(256, 256 - 30, 30), (200, 200 - 17, 17), (130, 130 - 9, 9), (130, 130 - 30, 30), (200, 200 - 1, 1)]   # c0 + b == ncols
assert any(c0 % 64 and c0 % 64 + b > 64 for _, c0, b in WINDOWS) and any(c0 % 64 + b <= 64 for _, c0, b in WINDOWS)   # across a word, and not


@pytest.mark.parametrize("case", WINDOWS, ids=lambda c: "%d-c%d-b%d" % c)
def test_windows(dev, L, case):
    ncols, c0, b = case
    NA, NB = (150, 130) if b < 8 else (R + 5, 700)           # few classes: few rows, or the pairs are too many
    ka, kb = drawn(NA, NB, b, NA // 3, 100 + c0 + b)
    if b >= 8:
        ka[::7] ^= 1 << (b - 1)                # the highest bit of the key, which only the last pass sees
        kb[::5] ^= 1 << (b - 1)
    wa, wb = keyed(NA, ncols, c0, b, ka, 200 + c0 + b), keyed(NB, ncols, c0, b, kb, 300 + c0 + b)
    count, want = run(dev, L, wa, wb, ncols, c0, b, layouts=(OO, EE, OE) if c0 else (EE, OE, EE))
    assert count > 100 and (b == 0 or not keys(want.D, c0, b).any())      # the window of D is zero


# ---- key distributions -------------------------------------------------------------------------------------------------------------

def test_keys_on_one_side_only(dev, L):
    ncols, c0, b = 128, 33, 16
    rng = np.random.default_rng(1)
    ka = rng.permutation(np.concatenate([np.full(40, 5), np.full(30, 900), np.arange(100, 400), np.full(20, 60000)]))     # 100 .. 399, 60000: A only
    kb = rng.permutation(np.concatenate([np.full(25, 5), np.full(35, 900), np.arange(1000, 1500), np.full(10, 2)]))       # 1000 .. 1499, 2: B only
    count, want = run(dev, L, keyed(len(ka), ncols, c0, b, ka, 1), keyed(len(kb), ncols, c0, b, kb, 2), ncols, c0, b)
    assert count == 40 * 25 + 30 * 35


def test_all_keys_equal(dev, L):
    """one class on either side; R + 100 rows of A: every position of the second run has every row of B for a partner"""
    NA, NB, ncols, c0, b = R + 100, 70, 64, 20, 12
    wa, wb = keyed(NA, ncols, c0, b, np.full(NA, 0xABC), 1), keyed(NB, ncols, c0, b, np.full(NB, 0xABC), 2)
    count, want = run(dev, L, wa, wb, ncols, c0, b, layouts=(EO, EE, EE))
    assert count == NA * NB and (want.ia[-1], want.ib[-1]) == (NA - 1, NB - 1)
    assert run(dev, L, wa[:90], wb, ncols, c0, 0)[0] == 90 * NB               # b == 0: one class whatever the bits say


def test_all_keys_distinct_and_equal_across(dev, L):
    N, ncols, c0, b = 2 * R + 5, 256, 37, 14
    rng = np.random.default_rng(2)
    k = rng.permutation(1 << b)[:N]
    wa, wb = keyed(N, ncols, c0, b, k, 2), keyed(N, ncols, c0, b, k[rng.permutation(N)], 3)
    count, want = run(dev, L, wa, wb, ncols, c0, b)
    assert count == N and len(set(want.ia)) == N and len(set(want.ib)) == N


def test_no_key_in_common(dev, L):
    NA, NB, ncols, c0, b = R + 9, 500, 130, 64, 12
    rng = np.random.default_rng(3)
    wa, wb = keyed(NA, ncols, c0, b, 2 * rng.integers(0, 2000, NA), 4), keyed(NB, ncols, c0, b, 2 * rng.integers(0, 2000, NB) + 1, 5)
    assert run(dev, L, wa, wb, ncols, c0, b, cap=7)[0] == 0               # nothing is written
    assert run(dev, L, wa, wb, ncols, c0, b, cap="zero")[0] == 0
    # ... every key of B above, and every key of B below, every key of A
    assert run(dev, L, wa, keyed(NB, ncols, c0, b, np.full(NB, 4095), 6), ncols, c0, b, cap=3)[0] == 0
    assert run(dev, L, keyed(NA, ncols, c0, b, np.arange(NA) + 7, 7), keyed(NB, ncols, c0, b, np.arange(NB) % 7, 8), ncols, c0, b, cap=3)[0] == 0


def test_a_class_of_a_straddles_a_run_boundary(dev, L):
    """R - 20 rows of distinct keys, then a class of 50 that begins in the first run and ends in the second"""
    ncols, c0, b = 128, 33, 16
    ka = np.concatenate([np.arange(R - 20), np.full(50, R + 5), np.arange(200) + 2 * R])
    kb = np.concatenate([np.full(3, R + 5), np.arange(0, R, 3), np.full(2, 2 * R + 199), np.full(4, 7)])
    rng = np.random.default_rng(8)
    ka, kb = ka[rng.permutation(len(ka))], kb[rng.permutation(len(kb))]
    sa = np.sort(ka)
    assert sa[R - 20] == sa[R - 1] == sa[R] == sa[R + 29] == R + 5
    count, _ = run(dev, L, keyed(len(ka), ncols, c0, b, ka, 8), keyed(len(kb), ncols, c0, b, kb, 9), ncols, c0, b)
    before = len(np.arange(0, R - 20, 3)) + 4          # the outputs of the distinct keys in front of the class: key 7 meets four rows
    assert count == before + 150 + 2
    run(dev, L, keyed(len(ka), ncols, c0, b, ka, 8), keyed(len(kb), ncols, c0, b, kb, 9), ncols, c0, b, cap=before + 70)    # cut inside the class


@pytest.mark.parametrize("span", ["S", "S+7"])
def test_classes_of_b_at_the_end_of_the_staged_span(dev, L, span):
    """the sorted keys of B: 5 of key 10, fillers that A does not hold, 8 of key 20 that END at position S - 1 of the run's span, 7 of
    key 30 that BEGIN at position S.  A holds 10 and 20: the span is S keys and is staged in LDS; with 30 as well it is S + 7 keys
    and is bisected in global memory"""
    ncols, c0, b = 100, 40, 8
    kb = np.concatenate([np.full(5, 10), np.full(S - 13, 12), np.full(8, 20), np.full(7, 30), np.full(6, 3), np.full(9, 200)])
    sb = np.sort(kb)
    at = int(np.searchsorted(sb, 10))         # where the span begins
    assert sb[at + S - 9] == 12 and sb[at + S - 8] == sb[at + S - 1] == 20 and sb[at + S] == sb[at + S + 6] == 30 and sb[at + S + 7] == 200
    ka = np.concatenate([np.full(3, 10), np.full(4, 20), np.full(2, 30) if span == "S+7" else np.full(2, 25)])     # 25: in no row of B
    rng = np.random.default_rng(9)
    ka, kb = ka[rng.permutation(len(ka))], kb[rng.permutation(len(kb))]
    count, _ = run(dev, L, keyed(len(ka), ncols, c0, b, ka, 10), keyed(len(kb), ncols, c0, b, kb, 11), ncols, c0, b, layouts=(EE, OO, EE))
    assert count == 3 * 5 + 4 * 8 + (2 * 7 if span == "S+7" else 0)


def test_b_much_larger_than_a_with_a_giant_class(dev, L):
    """NB = 40 NA, random keys, and one class of B of 3 S rows: the span of every run leaves LDS"""
    NA, ncols, c0, b = 400, 64, 11, 12
    NB = 40 * NA
    assert NB > 3 * S + 1000
    rng = np.random.default_rng(12)
    ka, kb = rng.integers(0, 1 << b, NA), rng.integers(0, 1 << b, NB)
    kb[rng.permutation(NB)[:3 * S]] = 0x777
    ka[[5, 300]] = 0x777
    count, _ = run(dev, L, keyed(NA, ncols, c0, b, ka, 12), keyed(NB, ncols, c0, b, kb, 13), ncols, c0, b)
    assert count >= 2 * 3 * S


def test_a_self_join(dev, L):
    """A and B are one view: all ordered pairs of a class, (i, i) included, which are zero rows"""
    N, ncols, c0, b = R + 40, 130, 100, 9
    wa = keyed(N, ncols, c0, b, drawn(N, N, b, N // 4, 14)[0], 14)
    count, want = run(dev, L, wa, wa, ncols, c0, b, same=True, layouts=(OO, OO, EE))
    sizes = np.unique(keys(wa, c0, b), return_counts=True)[1]
    same = want.ia == want.ib
    assert count == int((sizes * sizes).sum()) and same.sum() == N and not want.D[same].any() and not want.wt[same].any()


# ---- row widths and alignment ------------------------------------------------------------------------------------------------------

WIDTHS = [1, 64, 65, 130, 200, 256, 257, 320, 513, 1030, 4100]


def test_the_widths_cover_the_lanes(dev):
    lanes = {dev.join_plan(100, 100, n, 4)[3] for n in WIDTHS}
    assert lanes == {dev.join_plan(100, 100, n, 4)[3] for n in range(4, 8200, 61)} == {1, 2, 8, 64}
    assert any(n % 64 for n in WIDTHS) and any(n % 64 == 0 for n in WIDTHS) and any(g.width(n) % 2 for n in WIDTHS)


@pytest.mark.parametrize("layouts", LAYOUT_TRIPLES, ids=lambda t: "A%d%d-B%d%d-D%d%d" % (t[0] + t[1] + t[2]))
@pytest.mark.parametrize("ncols", WIDTHS)
def test_widths_and_alignment(dev, L, ncols, layouts):
    b = min(5, ncols)
    c0 = ncols - b               # the window ends with the row
    NA, NB = (R + 77, 150) if ncols >= 5 else (90, 80)    # two runs
    wa, wb = pools(NA, NB, ncols, c0, b, 20, ncols)
    wb[NB - 3] = wa[2]           # a repeated row: a zero row in D
    lo = min(3, ncols - 1)
    count, want = run(dev, L, wa, wb, ncols, c0, b, cap="more", layouts=layouts, wcols=(lo, ncols))
    t = list(zip(want.ia, want.ib)).index((2, NB - 3))
    assert not want.D[t].any() and want.wt[t] == 0
    run(dev, L, wa, wb, ncols, c0, b, cap="less", layouts=layouts, given=("ia", "wt"), wcols=(0, ncols - b))


# ---- capacity ----------------------------------------------------------------------------------------------------------------------

def capacity_pools():
    ncols, c0, b = 257, 250, 4
    return g.random_words(500, ncols, 55), g.random_words(400, ncols, 56), ncols, c0, b


SUBSETS = [tuple(s) for r in range(4) for s in itertools.combinations(ARRAYS, r)]


@pytest.mark.parametrize("given", SUBSETS, ids=lambda s: "+".join(s) or "none")
@pytest.mark.parametrize("cap", ["zero", 1, "count-1", "equal", "more", "in a position"])
def test_capacity(dev, L, cap, given):
    wa, wb, ncols, c0, b = capacity_pools()
    ka, kb = keys(wa, c0, b), keys(wb, c0, b)
    count = jr.pair_count(ka, kb)
    first = np.sort(ka)[0]
    na0, nb0 = int((ka == first).sum()), int((kb == first).sum())
    assert na0 >= 3 and nb0 >= 5 and count > 5000
    capn = {"count-1": count - 1, "in a position": 2 * nb0 + 3}.get(cap, cap)     # inside the outputs of the third member of the first class
    got, want = run(dev, L, wa, wb, ncols, c0, b, cap=capn, given=given, layouts=(OO, EE, OE), wcols=(10, 250))
    assert got == count
    if cap == "in a position":
        assert want.ia[-1] == want.ia[-3] != want.ia[-4] and list(want.ib[-3:]) == sorted(want.ib[-3:])


# ---- weight ranges -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wcols", [(0, 0), (77, 77), (200, 200), (0, 200), (70, 100), (60, 140), (3, 193), (129, 200), (191, 200)],
                         ids=lambda w: "%d-%d" % w)
def test_weight_ranges(dev, L, wcols):
    """empty, the whole row, inside one word, across three words, ending at ncols with ncols % 64 != 0"""
    ncols, c0, b = 200, 90, 6
    wa, wb = pools(300, 200, ncols, c0, b, 30, 77)
    count, want = run(dev, L, wa, wb, ncols, c0, b, wcols=wcols, layouts=(EO, OE, EE))
    bits = g.words_to_bits(want.D, ncols)
    assert count > 500 and np.array_equal(want.wt, bits[:, wcols[0]:wcols[1]].sum(axis=1))
    if wcols[1] > wcols[0] + 20:
        assert want.wt.max() > want.wt.min()


# ---- the count ---------------------------------------------------------------------------------------------------------------------

def test_a_count_past_2_to_31(dev, L):
    """50 000 rows of one key on either side: 2 500 000 000 pairs.  1000 of them are written; the count-only form says the same"""
    N, ncols, c0, b = 50000, 96, 70, 21
    wa, wb = keyed(N, ncols, c0, b, np.full(N, 0x12345), 70), keyed(N, ncols, c0, b, np.full(N, 0x12345), 71)
    count, want = run(dev, L, wa, wb, ncols, c0, b, cap=1000, layouts=(EE, OO, OO))
    assert count == 2500000000 > 1 << 31 and len(want.ia) == 1000
    assert run(dev, L, wa, wb, ncols, c0, b, cap="zero")[0] == count


@pytest.mark.parametrize("b", [8, 12])
def test_random_keys(dev, L, b):
    """NA = NB = 3 * 2^b: the pair indicators are pairwise independent, so the count has the variance NA NB p (1 - p), p = 2^-b"""
    N, ncols, c0 = 3 << b, 256, 101
    wa, wb = g.random_words(N, ncols, b), g.random_words(N, ncols, b + 100)
    mean = N * N / (1 << b)
    assert abs(jr.pair_count(keys(wa, c0, b), keys(wb, c0, b)) - mean) <= 6 * np.sqrt(mean)      # the yardstick's count first
    count, _ = run(dev, L, wa, wb, ncols, c0, b)
    assert abs(count - mean) <= 6 * np.sqrt(mean)


# ---- the wrappers, composition -----------------------------------------------------------------------------------------------------

def test_wrappers_size_their_results(dev):
    NA, NB, ncols, c0, b = 3000, 2000, 100, 41, 10
    wa, wb = g.random_words(NA, ncols, 8), g.random_words(NB, ncols, 9)
    want = jr.join(wa, wb, ncols, c0, b, 20, 90)
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    D, count, ia, ib, wt = dev.join(A, B, c0, b, wcols=(20, 90))          # cap=None: a count-only call first
    assert D.nrows == want.count == len(want.ia) and np.array_equal(D.to_words(), want.D)
    assert int(count.read(None)[0]) == D.nrows and count.read(None).dtype == np.int64
    assert np.array_equal(ia.read(None), want.ia) and np.array_equal(ib.read(None), want.ib) and np.array_equal(wt.read(None), want.wt)
    D = A.join(B, c0, b)
    assert D.nrows == want.count and np.array_equal(D.to_words(), want.D)
    D, wt = A.join(B, c0, b, wcols=(20, 90))
    assert np.array_equal(D.to_words(), want.D) and np.array_equal(wt.read(None), want.wt)
    whole = dev.join(A, B, c0, b, ia=dev.SKIP, ib=dev.SKIP)
    assert whole[2] is None and whole[3] is None and np.array_equal(whole[4].read(None), jr.weights(want.D, 0, ncols))
    # no pair: an empty matrix
    E = dev.DMat.from_words(wa[:1], ncols).join(dev.DMat.wrap(None, 0, ncols, 2), c0, b)
    assert E.nrows == 0 and E.ncols == ncols
    assert np.array_equal(A.to_words(), wa) and np.array_equal(B.to_words(), wb)


def test_ia_and_ib_feed_the_gathers(dev):
    """D == gather(A, ia) ^ gather(B, ib): the index outputs go to the gathers as the device arrays they are"""
    NA, NB, ncols, c0, b = 5000, 4000, 300, 100, 11
    wa, wb = g.random_words(NA, ncols, 17), g.random_words(NB, ncols, 18)
    want = jr.join(wa, wb, ncols, c0, b)
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    D, count, ia, ib, wt = dev.join(A, B, c0, b, cap=want.count, wt=dev.SKIP)
    D2 = dev.DMat(want.count, ncols)
    dev.gather_rows(A, ia.ptr, D=D2)
    dev.gather_rows(B, ib.ptr, D=D2, accumulate=True)
    assert wt is None and np.array_equal(D2.to_words(), want.D) and np.array_equal(D.to_words(), want.D)


def test_two_calls_give_the_same_bits(dev, L):
    NA, NB, ncols, c0, b = 3 * R + 1, 2 * R + 7, 192, 77, 11
    wa, wb = g.random_words(NA, ncols, 21), g.random_words(NB, ncols, 22)
    A, B = dev.DMat.from_words(wa, ncols), dev.DMat.from_words(wb, ncols)
    results = []
    for _ in range(2):
        D, count, ia, ib, wt = dev.join(A, B, c0, b, cap=3 * NA)
        n = int(count.read(None)[0])
        results.append((n, D.to_words()[:n], ia.read(None)[:n], ib.read(None)[:n], wt.read(None)[:n]))
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    assert results[0][0] == jr.pair_count(keys(wa, c0, b), keys(wb, c0, b)) <= 3 * NA


# ---- dirty scratch, streams, past 4 GiB --------------------------------------------------------------------------------------------

def test_on_dirty_scratch(dev, L):
    """the sorts' work space, the sorted orders and keys of A and B and the run sums come from a cache in which every block holds a
    pattern, and no block comes fresh from the driver"""
    import torch
    for pattern in dp.PATTERNS:
        cache = dp.Pool(L, pattern)
        for NA, NB, ncols, b in ((3 * R + 5, 2000, 128, 9), (2 * R + 77, 5 * S + 9, 320, 25), (700, 900, 64, 0)):
            wa, wb = pools(NA, NB, ncols, 33, b, NA // 3, NA)
            stream = torch.cuda.Stream().cuda_stream     # a caller stream: its arena is new
            h0 = cache.hits()
            run(dev, L, wa, wb, ncols, 33, b, stream=stream, cap=20000 if b == 0 else "more")
            assert cache.hits() - h0 >= 1
            cache.no_fresh("the join on dirty scratch")
    gc.collect()
    L.gf2_trim()


def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pools are written by gf2_dmat_fill_random on the caller's stream, behind a sleep; the same join is enqueued twice behind
    it, into two destinations, before anything synchronises.  Both must hold what the yardstick makes of the seeded pools."""
    import torch
    NA, NB, ncols, c0, b, seed = 9001, 7003, 200, 57, 12, 0xB1C
    wa, wb = lr.seeded_words(seed, ncols, np.arange(NA)), lr.seeded_words(seed + 1, ncols, np.arange(NB))
    want = jr.join(wa, wb, ncols, c0, b, 0, 57)
    count = want.count
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    ta = torch.full((NA, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    tb = torch.full((NB, 4), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    A, B = dev.DMat.from_torch(ta, ncols), dev.DMat.from_torch(tb, ncols)
    outs = []
    for _ in range(2):
        td = torch.full((count + 2, 4), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.from_torch(td, ncols), guarded(2), guarded(count + 2), guarded(count + 2), guarded(count + 2)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(100_000_000)
    A.fill_random(seed, s)
    B.fill_random(seed + 1, s)
    for td, D, (tc, pc), (ti, pi), (tj, pj), (tw, pw) in outs:
        dev.join(A, B, c0, b, D=D, count=pc, ia=pi, ib=pj, wt=pw, wcols=(0, 57), stream=s)
    pending = not stream.query()
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for td, D, (tc, pc), (ti, pi), (tj, pj), (tw, pw) in outs:
        rows = td.cpu().numpy().view(np.uint64)
        assert count_of(tc) == count
        assert np.array_equal(rows[:count], want.D) and np.all(rows[count:] == np.uint64(0x1111111111111111))
        assert np.array_equal(read_guarded(ti)[:count], want.ia) and np.array_equal(read_guarded(tj)[:count], want.ib)
        assert np.array_equal(read_guarded(tw)[:count], want.wt)


def test_a_view_of_a_parent_past_4gib(dev, L):
    """A: 70 000 rows of 128 columns, 8192 words apart: its last rows start behind byte offset 2^32 of the parent.  Only the view's
    words are written (gf2_copy_block_dev from a compact upload); B and D are compact"""
    import torch
    NA, NB, ncols, ld, c0, b = 70000, 3000, 128, 8192, 60, 15
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((NA, ld), dtype=torch.int64, device="cuda")
    assert NA * ld * 8 > lr.LIMIT_BYTES
    wa, wb = g.random_words(NA, ncols, 70), g.random_words(NB, ncols, 71)
    r_hi = lr.straddle(ld, NA)[1]
    wb[5] = wa[NA - 1]                            # a pair whose row of A lies behind 2^32: a zero row
    A = dev.DMat.wrap(t.data_ptr() + 8 * 6, NA, ncols, ld, keep=t)
    dev.copy_block(A, 0, 0, dev.DMat.from_words(wa, ncols), 0, 0, NA, ncols)
    B = dev.DMat.from_words(wb, ncols)
    want = jr.join(wa, wb, ncols, c0, b, 64, 128)
    D, count, ia, ib, wt = dev.join(A, B, c0, b, cap=want.count + 1, wcols=(64, 128))
    assert int(count.read(None)[0]) == want.count
    assert np.array_equal(ia.read(None)[:-1], want.ia) and np.array_equal(ib.read(None)[:-1], want.ib)
    assert np.array_equal(wt.read(None)[:-1], want.wt) and np.array_equal(D.to_words()[:-1], want.D)
    assert (want.ia > r_hi).sum() > 0 and not want.D[list(zip(want.ia, want.ib)).index((NA - 1, 5))].any()
    del t, A, D
    gc.collect()
    torch.cuda.empty_cache()


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def stern_instance(seed):
    """Q: 128 x 400 random bits.  The error has one column in each half of Q (i, 200 + j) and 5 more ones among the rows 8 .. 127 (e1);
    s = Q[:, i] ^ Q[:, 200 + j] ^ e1 -> (Q, s, i, j, e1), all as bits"""
    rng = np.random.default_rng(seed)
    Q = rng.integers(0, 2, (128, 400), dtype=np.uint8)
    i, j = int(rng.integers(0, 200)), int(rng.integers(0, 200))
    e1 = np.zeros(128, dtype=np.uint8)
    e1[rng.choice(np.arange(8, 128), 5, replace=False)] = 1
    return Q, Q[:, i] ^ Q[:, 200 + j] ^ e1, i, j, e1


def stern_pools(seed):
    Q, s, i, j, e1 = stern_instance(seed)
    wa = g.bits_to_words(np.ascontiguousarray(Q[:, :200].T) ^ s[None, :])
    wb = g.bits_to_words(np.ascontiguousarray(Q[:, 200:].T))
    return Q, s, i, j, e1, wa, wb


@pytest.mark.parametrize("seed", range(6))
def test_stern_collision_end_to_end(dev, seed):
    """a Stern collision with p = 1: A = the 200 columns of the left half of Q, each ^ s, B = those of the right half, as rows; the
    join on the columns [0, 8) with the weights over [8, 128), the selection of the weights up to 5, the gather of the hits -- one
    chain, one synchronisation at its end.  The planted pair is the only hit"""
    import torch
    Q, s, i, j, e1, wa, wb = stern_pools(seed)
    want = jr.join(wa, wb, 128, 0, 8, 8, 128)
    light = np.flatnonzero(want.wt <= 5)
    assert 134 <= want.count <= 174 and len(light) == 1 and np.sort(want.wt)[1] >= 41          # the yardstick alone finds the pair, and only it
    t = int(light[0])
    assert (want.ia[t], want.ib[t]) == (i, j) and np.array_equal(g.words_to_bits(want.D[t:t + 1], 128)[0], e1)
    # A and B on the device: Q goes up once, is transposed, cut in two, and s is XORed into every row of the left half
    Qt = dev.transpose(dev.DMat.from_words(g.bits_to_words(Q), 400))
    A = dev.submatrix(Qt, 0, 0, 200, 128)
    B = dev.submatrix(Qt, 200, 0, 400, 128)
    srows = dev.DMat.from_words(np.tile(g.bits_to_words(s[None, :]), (200, 1)), 128)
    dev.copy_block(A, 0, 0, srows, 0, 0, 200, 128, accumulate=True)
    cap = 400
    ti, pi = guarded(4)
    tn, pn = guarded(1)
    hit = dev.DMat(1, 128)
    torch.cuda.synchronize()
    D, count, ia, ib, wt = dev.join(A, B, 0, 8, cap=cap, wcols=(8, 128))
    dev.select_weights(wt.ptr, want.count, 0, 5, idx=pi, cap=4, count=pn)
    dev.gather_rows(D, pi, D=hit)                      # the first hit
    torch.cuda.synchronize()
    assert int(count.read(None)[0]) == want.count <= cap
    assert np.array_equal(A.to_words(), wa) and np.array_equal(B.to_words(), wb)
    assert np.array_equal(D.to_words()[:want.count], want.D) and np.array_equal(wt.read(None)[:want.count], want.wt)
    assert int(read_guarded(tn)[0]) == 1 and int(read_guarded(ti)[0]) == t
    assert (int(ia.read(None)[t]), int(ib.read(None)[t])) == (i, j)
    assert np.array_equal(g.words_to_bits(hit.to_words(), 128)[0], e1)
