"""CPU tests of the contract of include/m4ri_hip_join_select.h (gf2_join_select_dev, gf2_join_select_plan): every argument is checked
before a device is required and before the first HIP call, so this runs without one, on DMatStructs around addresses that are never
dereferenced (the BASE / FAR technique of tests/test_join_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.JOIN_SELECT_SYMBOLS) names exactly those;
the tables of the older headers do not, and are what they were."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_join_select.h")

BASE = 1 << 20     # A: an address that is never dereferenced
OTHER = 1 << 24    # B
FAR = 1 << 28      # D
COUNT = 1 << 29
HITS = (1 << 29) + (1 << 19)
IA = (1 << 29) + (1 << 20)
IB = (1 << 29) + (2 << 20)
WT = (1 << 29) + (3 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

SELECT, PLAN = "gf2_join_select_dev", "gf2_join_select_plan"
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


def select(L, pkg, A=DEFAULT, B=DEFAULT, D=DEFAULT, c0=37, b=20, wc0=57, wc1=200, wlo=0, whi=9, count=COUNT, hits=HITS, ia=IA, ib=IB, wt=WT):
    A = mat(pkg, 10, 200) if A is DEFAULT else A
    ncols = A.ncols if A is not None else 200
    B = mat(pkg, 12, ncols, OTHER) if B is DEFAULT else B
    D = mat(pkg, 10, ncols, FAR) if D is DEFAULT else D
    return L.gf2_join_select_dev(ref(D), ref(A), ref(B), c0, b, wc0, wc1, wlo, whi, count, hits, ia, ib, wt, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(SELECT) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_join_select.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_join_select_plan(1, 1, 1, 31, 0, 1, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {SELECT, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.JOIN_SELECT_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS, pkg._lib.JOIN_SYMBOLS, pkg._lib.SUMS_SYMBOLS):
        assert not declared & set(table)
    # ... and stay what they were
    assert set(pkg._lib.JOIN_SYMBOLS) == {"gf2_join_dev", "gf2_join_plan"}
    assert set(pkg._lib.SUMS_SYMBOLS) == {"gf2_subset_sums_dev", "gf2_unrank_subsets_dev", "gf2_subset_count", "gf2_subset_rank",
                                          "gf2_subset_unrank", "gf2_subset_sums_plan"}
    assert set(pkg._lib.LF2_SYMBOLS) == {"gf2_class_sort_dev", "gf2_lf2_reduce_dev", "gf2_lf2_plan"}
    # the argument lists are the issue's
    names = lambda decl: [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")]  # noqa: E731
    assert names(declarations()[SELECT]) == ["D", "A", "B", "c0", "b", "wc0", "wc1", "wlo", "whi", "count", "hits", "ia", "ib", "wt", "stream"]
    assert names(declarations()[PLAN]) == ["nrows_a", "nrows_b", "ncols", "b", "wc0", "wc1", "out"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("The pairs are those of gf2_join_dev, in its order", "ordered by (ia, ib)", "A pair is a HIT when wlo <= w(t) <= whi",
                  "for h < min(*hits, D->nrows)", "Nothing behind that is touched", "are not touched", "the same number as gf2_join_dev",
                  "may exceed 2^31", "*hits may exceed the capacity", "OVERWRITTEN", "bit for bit", "gf2_select_weights_dev(wt, count, wlo, whi",
                  "the gathers of D, ia, ib and wt by its indices", "The order is part of the contract", "No atomics are used",
                  "one writer per output word", "Two runs give the same bits", "D->data == NULL with D->nrows > 0 is allowed",
                  "gf2_subset_sums_dev", "index-only mode", "D->nrows == 0 writes only *count and *hits", "independently",
                  "0 <= wc0 <= wc1 <= ncols", "0 <= wlo <= whi", "whi may exceed the width of the range", "An empty range weighs 0",
                  "every pair is a hit when wlo == 0 and no pair otherwise", "b <= 30", "at most two words", "16-byte accesses are used only where",
                  "64-bit offsets", "never read", "by the rule of gf2_submatrix_dev", "A may be B", "(i, i) included",
                  "no host synchronisation and no hipMalloc", "from the slot of gf2_join_dev", "does not grow with the number of pairs",
                  "has been written by the same call", "before a device is required and before the first HIP call", "checked last", '"overlap"',
                  "they may overlap or be the identical view", "Nothing of A or B is written", "without a device", "no key in common"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_matrix_argument_errors(pkg, L):
    j = lambda **kw: select(L, pkg, **kw)  # noqa: E731
    for name, base in (("A", BASE), ("B", OTHER), ("D", FAR)):
        refused(L, j(**{name: None}), name + " is null")
        refused(L, j(**{name: mat(pkg, -1, 200, base)}), name, "negative")
        refused(L, j(**{name: mat(pkg, 10, 200, base, ld=width(200) - 1)}), name + ".ld is smaller")
        refused(L, j(**{name: mat(pkg, 10, 200, base + 4)}), name + ".data is not 8-byte aligned")
    for name in ("A", "B"):                                  # D alone may come without data
        refused(L, j(**{name: mat(pkg, 10, 200, None)}), name + ".data is null")
    refused(L, j(A=mat(pkg, 10, -200)), "negative")
    refused(L, j(B=mat(pkg, 12, 199, OTHER)), "must be equal")
    refused(L, j(B=mat(pkg, 12, 256, OTHER)), "must be equal")
    refused(L, j(D=mat(pkg, 10, 199, FAR)), "must be equal")
    refused(L, j(D=mat(pkg, 10, 256, None)), "must be equal")      # also without data


def test_window_counter_array_and_weight_errors(pkg, L):
    j = lambda **kw: select(L, pkg, **kw)  # noqa: E731
    for b in (-1, 31, 1 << 20):
        big = 1 << 21
        refused(L, j(A=mat(pkg, 10, big), b=b, wc1=big), "b = %d is outside 0 <= b <= 30" % b)
    refused(L, j(c0=-1), "c0", "outside A and B")
    refused(L, j(c0=181, b=20), "c0", "outside A and B")
    refused(L, j(c0=200, b=1), "c0", "outside A and B")
    refused(L, j(c0=(1 << 31) - 1, b=30), "c0", "outside A and B")
    refused(L, j(count=None), "count is null")
    refused(L, j(hits=None), "hits is null")
    refused(L, j(count=COUNT + 4), "count is not 8-byte aligned")
    refused(L, j(hits=HITS + 4), "hits is not 8-byte aligned")
    refused(L, j(hits=HITS + 1), "hits is not 8-byte aligned")
    refused(L, j(count=None, hits=None), "count is null")          # in the order of the arguments
    refused(L, j(ia=IA + 2), "ia is not 4-byte aligned")
    refused(L, j(ib=IB + 1), "ib is not 4-byte aligned")
    refused(L, j(wt=WT + 3), "wt is not 4-byte aligned")
    # the weight range
    refused(L, j(wc0=-1), "weight range", "[-1, 200)")
    refused(L, j(wc0=101, wc1=100), "weight range")
    refused(L, j(wc0=0, wc1=201), "weight range")
    refused(L, j(wc0=201, wc1=201), "weight range")
    refused(L, j(wc0=0, wc1=-1), "weight range")
    refused(L, j(wt=None, wc0=5, wc1=4), "weight range")
    # the weight window
    refused(L, j(wlo=-1), "weight window", "[-1, 9]")
    refused(L, j(wlo=5, whi=4), "weight window", "[5, 4]")
    refused(L, j(wlo=0, whi=-1), "weight window")
    refused(L, j(wlo=-3, whi=-2), "weight window")
    refused(L, j(wc0=9, wc1=8, wlo=5, whi=4), "weight range")      # the range is reported first
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, j())
        for skipped in ({"ia": None}, {"ib": None}, {"wt": None}, {"ia": None, "wt": None}, {"ia": None, "ib": None, "wt": None}):
            reaches_the_device_check(L, j(**skipped))
        reaches_the_device_check(L, j(wc0=0, wc1=0))                  # empty ranges, with a window that no pair meets
        reaches_the_device_check(L, j(wc0=200, wc1=200, wlo=1, whi=1))
        reaches_the_device_check(L, j(wc0=0, wc1=200))                # the whole row, the window included
        reaches_the_device_check(L, j(whi=(1 << 31) - 1))             # whi beyond the width of the range
        reaches_the_device_check(L, j(wlo=144, whi=500))
        reaches_the_device_check(L, j(wlo=7, whi=7))
        reaches_the_device_check(L, j(c0=180, b=20))
        reaches_the_device_check(L, j(c0=50, b=30))
        reaches_the_device_check(L, j(c0=200, b=0))
        reaches_the_device_check(L, j(D=mat(pkg, 0, 200, None)))      # the counts-only form
        reaches_the_device_check(L, j(D=mat(pkg, 0, 200, None), ia=None, ib=None, wt=None))
        reaches_the_device_check(L, j(D=mat(pkg, 10, 200, None)))     # the index-only mode: rows that are not stored
        reaches_the_device_check(L, j(D=mat(pkg, 10, 200, None), ia=None, wt=None))
        reaches_the_device_check(L, j(D=mat(pkg, 10, 200, None), ia=None, ib=None, wt=None))
        reaches_the_device_check(L, j(A=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, j(B=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, j(A=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))     # rows that are only 8-byte aligned
        reaches_the_device_check(L, j(B=mat(pkg, 12, 200, OTHER + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, j(D=mat(pkg, 10, 200, FAR + 8, ld=width(200) + 1)))


def test_a_and_b_may_overlap_or_be_one_view(pkg, L):
    A = mat(pkg, 10, 200, BASE, 6)
    j = lambda B, **kw: select(L, pkg, A=A, B=B, c0=0, b=4, **kw)  # noqa: E731
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, j(A))                                              # the identical view: a self-join
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE, 6)))
        reaches_the_device_check(L, j(mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)))
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE + 8 * 3, 6)))
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE + 8, 8)))
        reaches_the_device_check(L, j(A, D=mat(pkg, 10, 200, None, 6)))                # a D without data meets nothing
    refused(L, j(A, D=mat(pkg, 10, 200, BASE, 6)), "overlap", "D", "A")               # ... but D may not be one of them


def test_d_may_share_no_word_with_a_or_b(pkg, L):
    for name, base in (("A", BASE), ("B", OTHER)):
        M = mat(pkg, 10, 200, base, 6)
        j = lambda D, M=M, name=name, **kw: select(L, pkg, D=D, c0=0, b=4, **{name: M}, **kw)  # noqa: E731
        refused(L, j(mat(pkg, 10, 200, base, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 5, 200, base + 8 * 6 * 3, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 10, 200, base + 8 * 3, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 10, 200, base - 8 * 6 * 9, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 10, 200, base + 8, 8)), "overlap", "D", name)
        # bad arguments first: the overlap errors come last
        refused(L, j(mat(pkg, 10, 200, base, 6), count=COUNT + 4), "count is not 8-byte aligned")
        refused(L, j(mat(pkg, 10, 200, base, 6), hits=None), "hits is null")
        refused(L, j(mat(pkg, 10, 200, base, 6), wc0=9, wc1=8), "weight range")
        refused(L, j(mat(pkg, 10, 200, base, 6), wlo=9, whi=8), "weight window")
        if L.gf2_device_count() <= 0:
            reaches_the_device_check(L, j(mat(pkg, 10, 200, base + 8 * 6 * 10, 6)))          # right behind
            reaches_the_device_check(L, j(mat(pkg, 10, 200, base - 8 * 6 * 10, 6)))          # right before
            reaches_the_device_check(L, j(mat(pkg, 0, 200, None)))


def test_a_counter_or_an_array_inside_an_operand_is_refused(pkg, L):
    A = mat(pkg, 10, 200, BASE, 6)
    B = mat(pkg, 10, 200, OTHER, 6)
    D = mat(pkg, 10, 200, FAR, 6)
    end = lambda at: at + 8 * (9 * 6 + width(200))   # noqa: E731  the first byte behind the last word of a 10 x 200, ld 6
    j = lambda **kw: select(L, pkg, A=A, B=B, D=D, c0=0, b=4, **kw)  # noqa: E731
    for name, size, step in (("count", 8, 8), ("hits", 8, 8), ("ia", 40, 4), ("ib", 40, 4), ("wt", 40, 4)):
        for mname, m0 in (("A", BASE), ("B", OTHER), ("D", FAR)):
            for at in (m0, m0 + 8 * 6 + 8, end(m0) - step, m0 - size + step, m0 + 8 * 4):   # the pad words belong to the range
                refused(L, j(**{name: at}), "overlap", name, mname)
    # ... and against each other
    refused(L, j(count=COUNT, hits=COUNT), "overlap", "count", "hits")
    refused(L, j(count=IA, ia=IA), "overlap", "count", "ia")
    refused(L, j(hits=IA + 32, ia=IA), "overlap", "hits", "ia")
    refused(L, j(hits=IB + 32, ib=IB), "overlap", "hits", "ib")
    refused(L, j(hits=WT, wt=WT), "overlap", "hits", "wt")
    refused(L, j(count=WT + 32, wt=WT), "overlap", "count", "wt")
    refused(L, j(ia=IA, ib=IA), "overlap", "ia", "ib")
    refused(L, j(ia=IA, ib=IA + 36), "overlap", "ia", "ib")
    refused(L, j(ia=IA, wt=IA - 36), "overlap", "ia", "wt")
    refused(L, j(ib=IB, wt=IB + 4), "overlap", "ib", "wt")
    # bad arguments are reported before the overlap
    refused(L, select(L, pkg, A=A, B=B, D=D, c0=0, b=31, count=BASE), "b = 31")
    refused(L, j(ia=BASE, count=None), "count is null")
    refused(L, j(ia=BASE, hits=HITS + 2), "hits is not 8-byte aligned")
    refused(L, j(ia=BASE, wt=WT + 2), "wt is not 4-byte aligned")
    refused(L, j(ia=BASE, wc0=300, wc1=300), "weight range")
    refused(L, j(hits=BASE, wlo=3, whi=2), "weight window")
    # the index-only mode: the arrays still have D->nrows entries, though D itself meets nothing
    Dn = mat(pkg, 10, 200, None, 6)
    refused(L, select(L, pkg, A=A, B=B, D=Dn, c0=0, b=4, ia=BASE), "overlap", "ia", "A")
    refused(L, select(L, pkg, A=A, B=B, D=Dn, c0=0, b=4, ia=IA, wt=IA + 36), "overlap", "ia", "wt")
    if L.gf2_device_count() <= 0:
        for mname, m0 in (("A", BASE), ("B", OTHER), ("D", FAR)):
            reaches_the_device_check(L, j(ia=m0 - 40, count=end(m0), hits=end(m0) + 8, wt=end(m0) + 16))   # right before, right behind
        reaches_the_device_check(L, j(count=IA - 16, hits=IA - 8, ia=IA, ib=IA + 40, wt=IA + 80))            # side by side
        reaches_the_device_check(L, j(ia=None, ib=None, wt=None))
        reaches_the_device_check(L, select(L, pkg, A=A, B=B, D=mat(pkg, 0, 200, None), c0=0, b=4, ia=BASE, ib=BASE, wt=BASE))   # no room: empty arrays
        reaches_the_device_check(L, select(L, pkg, A=A, B=B, D=Dn, c0=0, b=4, ia=IA, ib=IA + 40, wt=IA + 80))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, na, nb, ncols, b, wc0, wc1):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_join_select_plan(na, nb, ncols, b, wc0, wc1, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    na, nb, ncols = 100003, 40007, 64 * 70
    assert [plan(L, na, nb, ncols, b, 0, 64)[0] for b in (0, 1, 8, 9, 30)] == [0, 1, 1, 2, 4]
    # the lanes of the weigh pass follow the WORDS of a row that hold a column of the range, wherever the range lies
    expected = {0: 1, 1: 1, 2: 1, 3: 2, 4: 2, 5: 8, 64: 8, 65: 64, 70: 64}
    for words, lanes in expected.items():
        for k0 in (0, 1, 70 - words):
            if k0 + words > 70:
                continue
            ranges = [(64 * k0, 64 * (k0 + words))]
            if words >= 2:
                ranges += [(64 * k0 + 63, 64 * (k0 + words - 1) + 1)]          # one column of the first and of the last word
            if words == 0:
                ranges = [(0, 0), (77, 77), (ncols, ncols)]
            for wc0, wc1 in ranges:
                passes, o = plan(L, na, nb, ncols, 9, wc0, wc1)
                assert passes == 2 and o[2] == lanes, (words, wc0, wc1, o)
                assert o[3] == 64                                                    # ... the row store by the row width: 70 words
    assert plan(L, na, nb, 4160, 9, 4100, 4130)[1][2:4] == [1, 64]                  # a wide row, a range inside one word
    assert plan(L, na, nb, 4160, 9, 63, 65)[1][2:4] == [1, 64]                      # two columns, two words
    for words in (1, 2, 3, 4, 5, 64, 65):
        n = 64 * words - 3
        for b in (0, 1, 8, 9, 30):
            passes, o = plan(L, na, nb, n, b, 0, min(n, 10))
            jp = device.join_plan(na, nb, n, b)
            threads, R, wlanes, lanes, lds, scratch, runs, G = o
            assert passes == jp[0] == -(-b // 8) and (threads, R, lanes, runs) == (jp[1], jp[2], jp[3], jp[7]), (o, jp)
            assert wlanes == 1 and lanes in (1, 2, 8, 64) and G * lanes == threads
            assert jp[5] < lds <= jp[5] + 64 and 2 * lds <= 160 * 1024               # the join's LDS and the waves' hits of a round
            assert scratch == jp[6] + 2 * ((8 * runs + 15) & ~15), (o, jp)           # the join's scratch + the hit sums, two int64 per run
            assert device.join_select_plan(na, nb, n, b, (0, min(n, 10))) == (passes,) + tuple(o)
    assert device.join_select_plan(10, 20, 200, 8) == device.join_select_plan(10, 20, 200, 8, (0, 200))
    assert plan(L, 0, 0, 256, 8, 0, 0)[0] == 1 and plan(L, 0, 5, 0, 0, 0, 0)[0] == 0
    for bad in ((-1, 5, 256, 8, 0, 9), (5, -1, 256, 8, 0, 9), (10, 10, -1, 8, 0, 0), (10, 10, 256, -1, 0, 9), (10, 10, 256, 31, 0, 9),
                (10, 10, 256, 8, -1, 9), (10, 10, 256, 8, 10, 9), (10, 10, 256, 8, 0, 257), (10, 10, 256, 8, 257, 257)):
        assert plan(L, *bad) == (-1, [-7] * 8), bad
        assert device.join_select_plan(*bad[:4], bad[4:]) is None
    assert L.gf2_join_select_plan(10, 10, 256, 20, 0, 256, None) == 3 and L.gf2_join_select_plan(10, 10, 256, 31, 0, 256, None) == -1
