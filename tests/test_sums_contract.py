"""CPU tests of the contract of include/m4ri_hip_sums.h (gf2_subset_sums_dev, gf2_unrank_subsets_dev, gf2_subset_sums_plan): every
argument is checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around
addresses that are never dereferenced (the BASE / FAR technique of tests/test_join_contract.py).  A call that has nothing to write
succeeds without a device.

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.SUMS_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import math
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_sums.h")

BASE = 1 << 20     # S: an address that is never dereferenced
OTHER = 1 << 24    # base
FAR = 1 << 28      # D
IDX = 1 << 29
WT = (1 << 29) + (1 << 20)
RANKS = (1 << 29) + (2 << 20)
BAD = (1 << 29) + (3 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

SUMS, UNRANK, PLAN = "gf2_subset_sums_dev", "gf2_unrank_subsets_dev", "gf2_subset_sums_plan"
HOST = {"gf2_subset_count", "gf2_subset_rank", "gf2_subset_unrank"}
DEFAULT = object()


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    return p


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def width(ncols):
    return (ncols + 63) // 64


def mat(pkg, nrows, ncols, data=BASE, ld=None):
    s = pkg._lib.DMatStruct()
    s.data, s.ld, s.nrows, s.ncols = data, ld if ld is not None else (width(ncols) + 1) & ~1, nrows, ncols
    return s


def sums(L, pkg, S=DEFAULT, base=DEFAULT, D=DEFAULT, p=2, rank0=3, idx=IDX, wt=WT, wc0=57, wc1=200):
    """20 rows of 200 columns, p = 2: 190 sums; D takes 10 of them from rank 3 on"""
    S = mat(pkg, 20, 200) if S is DEFAULT else S
    ncols = S.ncols if S is not None else 200
    base = mat(pkg, 1, ncols, OTHER) if base is DEFAULT else base
    D = mat(pkg, 10, ncols, FAR) if D is DEFAULT else D
    return L.gf2_subset_sums_dev(ref(D), ref(S), ref(base), p, rank0, idx, wt, wc0, wc1, None)


def unrank(L, ranks=RANKS, count=10, rank0=0, p=3, n=50, idx=IDX, bad=BAD):
    return L.gf2_unrank_subsets_dev(ranks, count, rank0, p, n, idx, bad, None)


def refused(L, rc, *words, entry=SUMS):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(entry) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


def device_free(L):
    return L.gf2_device_count() <= 0


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_sums.h"\nint main(void){ gf2_dmat d; long long o[6]; int c[4]; (void)d; '
                   'return gf2_subset_sums_plan(1, 1, 5, 0, o) != -1 || gf2_subset_count(4, 2) != 6 || gf2_subset_unrank(0, 2, c); }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {SUMS, UNRANK, PLAN} | HOST
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.SUMS_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS, pkg._lib.JOIN_SYMBOLS):   # stay what they were
        assert not declared & set(table)
    assert set(pkg._lib.JOIN_SYMBOLS) == {"gf2_join_dev", "gf2_join_plan"}
    # the argument lists are the issue's
    names = lambda fn: [a.split()[-1].lstrip("*").split("[")[0] for a in declarations()[fn].split(",")]  # noqa: E731
    assert names(SUMS) == ["D", "S", "base", "p", "rank0", "idx", "wt", "wc0", "wc1", "stream"]
    assert names(UNRANK) == ["ranks", "count", "rank0", "p", "n", "idx", "bad", "stream"]
    assert names(PLAN) == ["n", "ncols", "p", "count", "out"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("The order is part of the contract", "colexicographically", "C(c_1, 1) + C(c_2, 2) + ... + C(c_p, p)",
                  "does not depend on n", "must not pass 2^62", "the only legal call when n < p", "Rows not stored",
                  "and only here", "with both NULL the call returns -1", "an empty range gives 0", "gf2_select_weights_dev",
                  "by the rule of gf2_submatrix_dev", "Two runs give the same bits", "no atomics", "never read",
                  "16-byte accesses are used only where", "64-bit offsets", "rank0 may pass 2^32", "Nothing of S or base is written",
                  "no host synchronisation and no hipMalloc", "No scratch is needed", "before a device is required and before the first HIP call",
                  "checked last", '"overlap"', "they may overlap", "base may be a row of S's parent", "independently",
                  "never used as an address", "convention of gf2_gather_rows_dev", "what gf2_select_weights_dev leaves behind *count",
                  "without a device"):
        assert words in text, words


# ---- gf2_subset_sums_dev: arguments ---------------------------------------------------------------------------------------------------

def test_matrix_argument_errors(pkg, L):
    s = lambda **kw: sums(L, pkg, **kw)  # noqa: E731
    refused(L, s(S=None), "S is null")
    refused(L, s(D=None), "D is null")
    for name, base, rows in (("S", BASE, 20), ("base", OTHER, 1), ("D", FAR, 10)):
        refused(L, s(**{name: mat(pkg, -1, 200, base)}), name, "negative")
        refused(L, s(**{name: mat(pkg, rows, 200, base, ld=width(200) - 1)}), name + ".ld is smaller")
        refused(L, s(**{name: mat(pkg, rows, 200, base + 4)}), name + ".data is not 8-byte aligned")
    refused(L, s(S=mat(pkg, 20, 200, None)), "S.data is null")
    refused(L, s(base=mat(pkg, 1, 200, None)), "base.data is null")
    refused(L, s(S=mat(pkg, 20, -200)), "negative")
    # base is null or one row
    refused(L, s(base=mat(pkg, 2, 200, OTHER)), "base has 2 rows")
    refused(L, s(base=mat(pkg, 0, 200, None)), "base has 0 rows")
    # unequal column counts, either operand
    refused(L, s(base=mat(pkg, 1, 199, OTHER)), "must be equal")
    refused(L, s(base=mat(pkg, 1, 256, OTHER)), "must be equal")
    refused(L, s(D=mat(pkg, 10, 199, FAR)), "must be equal")
    refused(L, s(D=mat(pkg, 10, 256, FAR)), "must be equal")
    # rows not stored need an array
    refused(L, s(D=mat(pkg, 10, 200, None), idx=None, wt=None), "D.data is null", "idx or wt")


def test_p_count_window_weight_and_array_errors(pkg, L):
    s = lambda **kw: sums(L, pkg, **kw)  # noqa: E731
    for p in (0, -1, 5, 1 << 20):
        refused(L, s(p=p), "p = %d is outside 1 <= p <= 4" % p)
    # a count that overflows: C(n, p) past 2^62
    for n, p in ((102571, 4), (3024618, 3), ((1 << 31) - 1, 4)):
        assert math.comb(n, p) > 1 << 62
        refused(L, s(S=mat(pkg, n, 200), p=p), "C(%d, %d) passes 2^62" % (n, p), "overflows")
        refused(L, s(S=mat(pkg, n, 200), p=p, D=mat(pkg, 0, 200, None)), "passes 2^62")        # also where nothing is asked for
    # the window of ranks
    total = math.comb(20, 2)
    refused(L, s(rank0=-1), "ranks", "outside [0, C(n, p))")
    refused(L, s(rank0=total - 9), "ranks", "[0, %d)" % total)
    refused(L, s(rank0=total + 1, D=mat(pkg, 0, 200, None)), "ranks")
    refused(L, s(rank0=1 << 62), "ranks")
    refused(L, s(rank0=(1 << 63) - 1), "ranks")
    refused(L, s(S=mat(pkg, 1, 200), D=mat(pkg, 1, 200, FAR), rank0=0), "ranks", "[0, 0)")          # n < p: only an empty D is legal
    refused(L, s(S=mat(pkg, 3, 200), p=4, D=mat(pkg, 1, 200, FAR), rank0=0), "ranks", "[0, 0)")
    refused(L, s(idx=IDX + 2), "idx is not 4-byte aligned")
    refused(L, s(wt=WT + 1), "wt is not 4-byte aligned")
    # the weight range
    refused(L, s(wc0=-1), "weight range", "[-1, 200)")
    refused(L, s(wc0=101, wc1=100), "weight range")
    refused(L, s(wc0=0, wc1=201), "weight range")
    refused(L, s(wc0=201, wc1=201), "weight range")
    refused(L, s(wt=None, wc0=5, wc1=4), "weight range")           # also where no weight is asked for
    if device_free(L):
        reaches_the_device_check(L, s())
        for skipped in ({"idx": None}, {"wt": None}, {"idx": None, "wt": None}, {"base": None}):
            reaches_the_device_check(L, s(**skipped))
        reaches_the_device_check(L, s(wc0=0, wc1=0))                  # empty ranges
        reaches_the_device_check(L, s(wc0=200, wc1=200))
        reaches_the_device_check(L, s(wc0=0, wc1=200))
        reaches_the_device_check(L, s(rank0=0))
        reaches_the_device_check(L, s(rank0=total - 10))              # up to the last rank
        for p in (1, 3, 4):
            reaches_the_device_check(L, s(p=p, rank0=math.comb(20, p) - 10))
        # rows not stored: a null D.data with rows, while idx or wt is given
        reaches_the_device_check(L, s(D=mat(pkg, 10, 200, None)))
        reaches_the_device_check(L, s(D=mat(pkg, 10, 200, None), idx=None))
        reaches_the_device_check(L, s(D=mat(pkg, 10, 200, None), wt=None))
        reaches_the_device_check(L, s(D=mat(pkg, 10, 200, None, ld=0), wt=None))      # its ld says nothing
        # the largest n of p = 4, and a window far up: rank0 past 2^32
        reaches_the_device_check(L, s(S=mat(pkg, 102570, 200), p=4, rank0=math.comb(102570, 4) - 10))
        reaches_the_device_check(L, s(S=mat(pkg, 131072, 200), rank0=(1 << 32) + 5))
        # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
        reaches_the_device_check(L, s(S=mat(pkg, 20, 200, BASE + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, s(base=mat(pkg, 1, 200, OTHER + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, s(D=mat(pkg, 10, 200, FAR + 8, ld=width(200) + 1)))


def test_nothing_to_write_succeeds_without_a_device(pkg, L):
    s = lambda **kw: sums(L, pkg, **kw)  # noqa: E731
    total = math.comb(20, 2)
    assert s(D=mat(pkg, 0, 200, None)) == 0
    assert s(D=mat(pkg, 0, 200, None), rank0=total) == 0                          # an empty window at the very end
    assert s(D=mat(pkg, 0, 200, FAR), idx=None, wt=None, base=None) == 0
    for n, p in ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4)):                          # n < p: the only legal call
        assert s(S=mat(pkg, n, 200, BASE if n else None), p=p, D=mat(pkg, 0, 200, None), rank0=0) == 0
        refused(L, s(S=mat(pkg, n, 200, BASE if n else None), p=p, D=mat(pkg, 0, 200, None), rank0=1), "ranks")
    assert s(D=mat(pkg, 0, 200, None), idx=BASE, wt=BASE) == 0                     # empty arrays meet nothing


# ---- gf2_subset_sums_dev: aliasing ------------------------------------------------------------------------------------------------------

def test_s_and_base_may_overlap(pkg, L):
    S = mat(pkg, 20, 200, BASE, 6)
    s = lambda base, **kw: sums(L, pkg, S=S, base=base, **kw)  # noqa: E731
    if device_free(L):
        reaches_the_device_check(L, s(mat(pkg, 1, 200, BASE, 6)))                      # base is S's first row
        reaches_the_device_check(L, s(mat(pkg, 1, 200, BASE + 8 * 6 * 7 + 8, 6)))      # inside S, a word off
        reaches_the_device_check(L, s(mat(pkg, 1, 200, BASE + 8 * 6 * 20, 6)))         # the row of S's parent behind S
    refused(L, s(mat(pkg, 1, 200, BASE, 6), D=mat(pkg, 10, 200, BASE + 8 * 6 * 3, 6)), "overlap", "D", "S")


def test_d_may_share_no_word_with_s_or_base(pkg, L):
    for name, base, rows in (("S", BASE, 20), ("base", OTHER, 1)):
        M = mat(pkg, rows, 200, base, 6)
        s = lambda D, M=M, name=name, **kw: sums(L, pkg, D=D, **{name: M}, **kw)  # noqa: E731
        refused(L, s(mat(pkg, 10, 200, base, 6)), "overlap", "D", name)                      # in place
        refused(L, s(mat(pkg, 10, 200, base + 8 * 3, 6)), "overlap", "D", name)              # shifted by three words: shares one
        refused(L, s(mat(pkg, 10, 200, base - 8 * 6 * 9, 6)), "overlap", "D", name)          # its last row is the operand's first
        refused(L, s(mat(pkg, 10, 200, base + 8, 8)), "overlap", "D", name)                  # another ld: address ranges
        refused(L, s(mat(pkg, 10, 200, base, 6), idx=IDX + 2), "idx is not 4-byte aligned")  # bad arguments first
        refused(L, s(mat(pkg, 10, 200, base, 6), wc0=9, wc1=8), "weight range")
        refused(L, s(mat(pkg, 10, 200, base, 6), p=7), "p = 7")
        if device_free(L):
            reaches_the_device_check(L, s(mat(pkg, 10, 200, base + 8 * 6 * rows, 6)))        # right behind
            reaches_the_device_check(L, s(mat(pkg, 10, 200, base - 8 * 6 * 10, 6)))          # right before
            reaches_the_device_check(L, s(mat(pkg, 10, 200, None, 6)))                       # rows not stored share nothing
        assert s(mat(pkg, 0, 200, None)) == 0                                                # no room: D is empty
    refused(L, sums(L, pkg, S=mat(pkg, 20, 200, BASE, 6), D=mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)), "overlap", "D", "S")   # some of S's rows


def test_an_array_inside_an_operand_or_the_other_array_is_refused(pkg, L):
    S = mat(pkg, 20, 200, BASE, 6)
    base = mat(pkg, 1, 200, OTHER, 6)
    D = mat(pkg, 10, 200, FAR, 6)
    end = lambda at, rows: at + 8 * ((rows - 1) * 6 + width(200))   # noqa: E731  the first byte behind the last word
    for p in (1, 2, 4):
        s = lambda p=p, **kw: sums(L, pkg, S=S, base=base, D=D, p=p, rank0=0, **kw)  # noqa: E731
        for name, size in (("idx", 40 * p), ("wt", 40)):
            for mname, m0, rows in (("S", BASE, 20), ("base", OTHER, 1), ("D", FAR, 10)):
                for at in (m0, m0 + 8, end(m0, rows) - 4, m0 - size + 4) + ((m0 + 8 * 6 + 8, m0 + 8 * 4) if rows > 1 else ()):   # the pad words belong to the range
                    refused(L, s(**{name: at}), "overlap", name, mname)
        # ... and against each other: idx is D->nrows * p ints long
        refused(L, s(idx=IDX, wt=IDX), "overlap", "idx", "wt")
        refused(L, s(idx=IDX, wt=IDX + 40 * p - 4), "overlap", "idx", "wt")
        refused(L, s(idx=IDX, wt=IDX - 36), "overlap", "idx", "wt")
        if device_free(L):
            reaches_the_device_check(L, s(idx=IDX, wt=IDX + 40 * p))                         # side by side
            reaches_the_device_check(L, s(idx=IDX, wt=IDX - 40))
            for mname, m0, rows in (("S", BASE, 20), ("base", OTHER, 1), ("D", FAR, 10)):
                reaches_the_device_check(L, s(idx=m0 - 40 * p, wt=end(m0, rows)))            # right before, right behind
            reaches_the_device_check(L, sums(L, pkg, S=S, base=base, D=mat(pkg, 10, 200, None), p=p, rank0=0, idx=FAR, wt=FAR + 40 * p))
    s = lambda **kw: sums(L, pkg, S=S, base=base, D=D, **kw)  # noqa: E731
    # bad arguments are reported before the overlap
    refused(L, s(idx=BASE, p=0), "p = 0")
    refused(L, s(idx=BASE, wt=WT + 2), "wt is not 4-byte aligned")
    refused(L, s(idx=BASE, wc0=300, wc1=300), "weight range")
    refused(L, s(idx=BASE, rank0=10000), "ranks")


# ---- gf2_unrank_subsets_dev -------------------------------------------------------------------------------------------------------------

def test_unrank_argument_errors(pkg, L):
    r = lambda *words, **kw: refused(L, unrank(L, **kw), *words, entry=UNRANK)  # noqa: E731
    r("count is negative", count=-1)
    r("n is negative", n=-1)
    for p in (0, 5, -3):
        r("p = %d is outside" % p, p=p)
    r("passes 2^62", n=102571, p=4)
    r("rank0", rank0=-1)
    r("rank0", rank0=(1 << 62) + 1)
    r("ranks is null", ranks=None)
    r("idx is null", idx=None)
    r("ranks is not 4-byte aligned", ranks=RANKS + 2)
    r("idx is not 4-byte aligned", idx=IDX + 1)
    r("bad is not 4-byte aligned", bad=BAD + 2)
    # address ranges: ranks is count ints, idx count * p, bad one
    r("overlap", "ranks", "idx", idx=RANKS)
    r("overlap", "ranks", "idx", idx=RANKS + 36)
    r("overlap", "ranks", "idx", idx=RANKS - 4 * 3 * 10 + 4)
    r("overlap", "ranks", "bad", bad=RANKS + 36)
    r("overlap", "idx", "bad", bad=IDX + 4 * 3 * 10 - 4)
    r("idx is not 4-byte aligned", idx=RANKS + 1)                        # bad arguments first
    assert unrank(L, count=0) == 0 and unrank(L, count=0, ranks=None, idx=None, bad=None) == 0     # nothing to write: no device needed
    assert unrank(L, count=0, ranks=IDX, idx=IDX, bad=IDX) == 0
    if device_free(L):
        reaches_the_device_check(L, unrank(L))
        reaches_the_device_check(L, unrank(L, bad=None))
        reaches_the_device_check(L, unrank(L, idx=RANKS + 40, bad=RANKS + 40 + 120))          # side by side
        reaches_the_device_check(L, unrank(L, rank0=1 << 62, n=102570, p=4))
        reaches_the_device_check(L, unrank(L, n=2, p=3))                                      # no subset at all: every rank is bad


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, n, ncols, p, count):
    out = (ctypes.c_longlong * 6)(*([-7] * 6))
    return L.gf2_subset_sums_plan(n, ncols, p, count, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    lanes_by_width = []
    for words in (1, 2, 3, 4, 5, 64, 65):
        ncols = 64 * words - 3
        for p in (1, 2, 3, 4):
            for n in (p, 40, 500, 9000, 102570):
                total = math.comb(n, p)
                for count in sorted({0, 1, min(total, 1000), min(total, 5000000), min(total, (1 << 31) - 1)}):
                    kid, o = plan(L, n, ncols, p, count)
                    threads, R, lanes, lds, groups, scratch = o
                    what = (ncols, p, n, count, kid, o)
                    assert threads == 256 and scratch == 0 and lanes in (1, 2, 8, 64) and threads % lanes == 0, what
                    assert lanes == device.join_plan(100, 100, ncols, 4)[3], what                 # the thresholds of the join scatter
                    staged = 8 * words * (n + 1) <= 64 * 1024
                    assert kid == (0 if staged else 4) + (1, 2, 8, 64).index(lanes), what
                    assert (lds >= 8 * words * (n + 1) and 2 * lds <= 160 * 1024) if staged else lds == 0, what   # two workgroups per CU at the least
                    assert 1024 <= R <= 16384 and R & (R - 1) == 0 and groups == -(-count // R), what
                    assert R == 16384 or count // (2 * R) < 2048, what                            # R is halved only while the workgroups are few
                    assert device.subset_sums_plan(n, ncols, p, count) == (kid,) + tuple(o)
        lanes_by_width.append(lanes)
    assert lanes_by_width == sorted(lanes_by_width) and lanes_by_width[0] == 1 and lanes_by_width[-1] == 64
    # every id can be reached
    ids = {plan(L, n, ncols, 2, 100)[0] for ncols in (64, 200, 1000, 5000) for n in (20, 9000)}
    assert ids == set(range(8))
    for bad in ((-1, 256, 2, 0), (10, -1, 2, 1), (10, 256, 0, 1), (10, 256, 5, 1), (10, 256, 2, -1), (10, 256, 2, 46), (3, 256, 4, 1),
                (102571, 256, 4, 1), (131072, 64, 2, 1 << 31)):
        assert plan(L, *bad) == (-1, [-7] * 6), bad
        assert device.subset_sums_plan(*bad) is None
    assert plan(L, 10, 256, 2, 45)[0] == 1 and plan(L, 3, 256, 4, 0)[0] == 1              # all of them; n < p: the empty list
    assert L.gf2_subset_sums_plan(10, 256, 2, 45, None) == 1 and L.gf2_subset_sums_plan(10, 256, 5, 1, None) == -1
    assert device.subset_count(10, 2) == 45 and device.subset_count(2, 3) == 0 and device.subset_count(10, 5) is None
    assert device.subset_count(102571, 4) is None
