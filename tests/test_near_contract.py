"""CPU tests of the contract of include/m4ri_hip_near.h (gf2_near_pairs_dev, gf2_nearest_dev, gf2_near_plan): every argument is checked
before a device is required and before the first HIP call, so this runs without one, on DMatStructs around addresses that are never
dereferenced (the BASE / FAR technique of tests/test_join_select_contract.py, whose placements these are).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.NEAR_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_near.h")

BASE = 1 << 20     # A: an address that is never dereferenced
OTHER = 1 << 24    # B
FAR = 1 << 28      # D
HITS = (1 << 29) + (1 << 19)
IA = (1 << 29) + (1 << 20)
IB = (1 << 29) + (2 << 20)
WT = (1 << 29) + (3 << 20)
IDX, DIST = IA, IB
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

PAIRS, NEAREST, PLAN = "gf2_near_pairs_dev", "gf2_nearest_dev", "gf2_near_plan"
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


def pairs(L, pkg, A=DEFAULT, B=DEFAULT, D=DEFAULT, wc0=57, wc1=200, wlo=0, whi=9, flags=0, hits=HITS, ia=IA, ib=IB, wt=WT):
    A = mat(pkg, 10, 200) if A is DEFAULT else A
    ncols = A.ncols if A is not None else 200
    B = mat(pkg, 12, ncols, OTHER) if B is DEFAULT else B
    D = mat(pkg, 10, ncols, FAR) if D is DEFAULT else D
    return L.gf2_near_pairs_dev(ref(D), ref(A), ref(B), wc0, wc1, wlo, whi, flags, hits, ia, ib, wt, None)


def nearest(L, pkg, A=DEFAULT, B=DEFAULT, wc0=57, wc1=200, flags=0, idx=IDX, dist=DIST):
    A = mat(pkg, 10, 200) if A is DEFAULT else A
    ncols = A.ncols if A is not None else 200
    B = mat(pkg, 12, ncols, OTHER) if B is DEFAULT else B
    return L.gf2_nearest_dev(ref(A), ref(B), wc0, wc1, flags, idx, dist, None)


def refused(L, rc, *words, entry=PAIRS):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(entry) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_near.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_near_plan(1, 1, 1, 0, 2, o) != -1 || GF2_NEAR_OFF_DIAGONAL != 1 || GF2_NEAR_UPPER != 2; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {PAIRS, NEAREST, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.NEAR_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS, pkg._lib.JOIN_SYMBOLS, pkg._lib.SUMS_SYMBOLS,
                  pkg._lib.JOIN_SELECT_SYMBOLS):
        assert not declared & set(table)
    assert set(pkg._lib.JOIN_SELECT_SYMBOLS) == {"gf2_join_select_dev", "gf2_join_select_plan"}        # ... and stay what they were
    # the argument lists are the issue's
    names = lambda decl: [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")]  # noqa: E731
    assert names(declarations()[PAIRS]) == ["D", "A", "B", "wc0", "wc1", "wlo", "whi", "flags", "hits", "ia", "ib", "wt", "stream"]
    assert names(declarations()[NEAREST]) == ["A", "B", "wc0", "wc1", "flags", "idx", "dist", "stream"]
    assert names(declarations()[PLAN]) == ["nrows_a", "nrows_b", "ncols", "wc0", "wc1", "out"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("A pair is a HIT when it is admitted and wlo <= d(i, j) <= whi", "(ia ascending, then ib ascending)",
                  "for h < min(*hits, D->nrows)", "Nothing behind that is touched", "are not touched", "may exceed 2^31",
                  "*hits may exceed the capacity", "OVERWRITTEN", "bit for bit",
                  "gf2_join_select_dev(D, A, B, 0, 0, wc0, wc1, wlo, whi, &count, hits, ia, ib, wt, stream)",
                  "The order is part of the contract", "No atomics are used", "one writer per output word", "Two runs give the same bits",
                  "D->data == NULL with D->nrows > 0 is allowed", "index-only mode", "D->nrows == 0 writes only *hits", "independently",
                  "0 <= wc0 <= wc1 <= ncols", "0 <= wlo <= whi", "whi may exceed the width of the range", "An empty range weighs 0",
                  "16-byte accesses are used only where", "64-bit offsets", "never read", "by the rule of gf2_submatrix_dev", "A may be B",
                  "no host synchronisation and no hipMalloc", "from a slot of its own", "does not grow with the number of pairs",
                  "has been written by the same call", "before a device is required and before the first HIP call", "checked last",
                  '"overlap"', "they may overlap or be the identical view", "Nothing of A or B is written", "without a device",
                  "Unknown flag bits are refused", "idx[i] = -1 and dist[i] = -1", "the lowest j that attains it", "not both",
                  "does not depend on the order in which workgroups run", "a second launch folds the chunks"):
        assert words in text, words


# ---- arguments of gf2_near_pairs_dev -------------------------------------------------------------------------------------------------------

def test_matrix_argument_errors(pkg, L):
    j = lambda **kw: pairs(L, pkg, **kw)  # noqa: E731
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


def test_counter_array_weight_and_flag_errors(pkg, L):
    j = lambda **kw: pairs(L, pkg, **kw)  # noqa: E731
    refused(L, j(hits=None), "hits is null")
    refused(L, j(hits=HITS + 4), "hits is not 8-byte aligned")
    refused(L, j(hits=HITS + 1), "hits is not 8-byte aligned")
    refused(L, j(ia=IA + 2), "ia is not 4-byte aligned")
    refused(L, j(ib=IB + 1), "ib is not 4-byte aligned")
    refused(L, j(wt=WT + 3), "wt is not 4-byte aligned")
    refused(L, j(hits=None, ia=IA + 2), "hits is null")             # in the order of the arguments
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
    # unknown flags
    for flags in (4, 8, 7, -1, 1 << 30):
        refused(L, j(flags=flags), "flags = %d" % flags, "GF2_NEAR_OFF_DIAGONAL", "GF2_NEAR_UPPER")
    refused(L, j(flags=4, wlo=5, whi=4), "weight window")           # ... are reported behind the window
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, j())
        for flags in (0, 1, 2, 3):
            reaches_the_device_check(L, j(flags=flags))
        for skipped in ({"ia": None}, {"ib": None}, {"wt": None}, {"ia": None, "wt": None}, {"ia": None, "ib": None, "wt": None}):
            reaches_the_device_check(L, j(**skipped))
        reaches_the_device_check(L, j(wc0=0, wc1=0))                  # empty ranges, with a window that no pair meets
        reaches_the_device_check(L, j(wc0=200, wc1=200, wlo=1, whi=1))
        reaches_the_device_check(L, j(wc0=0, wc1=200))                # the whole row
        reaches_the_device_check(L, j(whi=(1 << 31) - 1))             # whi beyond the width of the range
        reaches_the_device_check(L, j(wlo=144, whi=500))
        reaches_the_device_check(L, j(wlo=7, whi=7))
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
    j = lambda B, **kw: pairs(L, pkg, A=A, B=B, **kw)  # noqa: E731
    if L.gf2_device_count() <= 0:
        for flags in (0, 1, 2):
            reaches_the_device_check(L, j(A, flags=flags))                             # the identical view
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE, 6)))
        reaches_the_device_check(L, j(mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)))
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE + 8 * 3, 6)))
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE + 8, 8)))
        reaches_the_device_check(L, j(A, D=mat(pkg, 10, 200, None, 6)))                # a D without data meets nothing
    refused(L, j(A, D=mat(pkg, 10, 200, BASE, 6)), "overlap", "D", "A")               # ... but D may not be one of them


def test_d_may_share_no_word_with_a_or_b(pkg, L):
    for name, base in (("A", BASE), ("B", OTHER)):
        M = mat(pkg, 10, 200, base, 6)
        j = lambda D, M=M, name=name, **kw: pairs(L, pkg, D=D, **{name: M}, **kw)  # noqa: E731
        refused(L, j(mat(pkg, 10, 200, base, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 5, 200, base + 8 * 6 * 3, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 10, 200, base + 8 * 3, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 10, 200, base - 8 * 6 * 9, 6)), "overlap", "D", name)
        refused(L, j(mat(pkg, 10, 200, base + 8, 8)), "overlap", "D", name)
        # bad arguments first: the overlap errors come last
        refused(L, j(mat(pkg, 10, 200, base, 6), hits=HITS + 4), "hits is not 8-byte aligned")
        refused(L, j(mat(pkg, 10, 200, base, 6), hits=None), "hits is null")
        refused(L, j(mat(pkg, 10, 200, base, 6), wc0=9, wc1=8), "weight range")
        refused(L, j(mat(pkg, 10, 200, base, 6), wlo=9, whi=8), "weight window")
        refused(L, j(mat(pkg, 10, 200, base, 6), flags=16), "flags = 16")
        if L.gf2_device_count() <= 0:
            reaches_the_device_check(L, j(mat(pkg, 10, 200, base + 8 * 6 * 10, 6)))          # right behind
            reaches_the_device_check(L, j(mat(pkg, 10, 200, base - 8 * 6 * 10, 6)))          # right before
            reaches_the_device_check(L, j(mat(pkg, 0, 200, None)))


def test_a_counter_or_an_array_inside_an_operand_is_refused(pkg, L):
    A = mat(pkg, 10, 200, BASE, 6)
    B = mat(pkg, 10, 200, OTHER, 6)
    D = mat(pkg, 10, 200, FAR, 6)
    end = lambda at: at + 8 * (9 * 6 + width(200))   # noqa: E731  the first byte behind the last word of a 10 x 200, ld 6
    j = lambda **kw: pairs(L, pkg, A=A, B=B, D=D, **kw)  # noqa: E731
    for name, size, step in (("hits", 8, 8), ("ia", 40, 4), ("ib", 40, 4), ("wt", 40, 4)):
        for mname, m0 in (("A", BASE), ("B", OTHER), ("D", FAR)):
            for at in (m0, m0 + 8 * 6 + 8, end(m0) - step, m0 - size + step, m0 + 8 * 4):   # the pad words belong to the range
                refused(L, j(**{name: at}), "overlap", name, mname)
    # ... and against each other
    refused(L, j(hits=IA + 32, ia=IA), "overlap", "hits", "ia")
    refused(L, j(hits=IB + 32, ib=IB), "overlap", "hits", "ib")
    refused(L, j(hits=WT, wt=WT), "overlap", "hits", "wt")
    refused(L, j(ia=IA, ib=IA), "overlap", "ia", "ib")
    refused(L, j(ia=IA, ib=IA + 36), "overlap", "ia", "ib")
    refused(L, j(ia=IA, wt=IA - 36), "overlap", "ia", "wt")
    refused(L, j(ib=IB, wt=IB + 4), "overlap", "ib", "wt")
    # bad arguments are reported before the overlap
    refused(L, j(ia=BASE, hits=None), "hits is null")
    refused(L, j(ia=BASE, hits=HITS + 2), "hits is not 8-byte aligned")
    refused(L, j(ia=BASE, wt=WT + 2), "wt is not 4-byte aligned")
    refused(L, j(ia=BASE, wc0=300, wc1=300), "weight range")
    refused(L, j(hits=BASE, wlo=3, whi=2), "weight window")
    refused(L, j(hits=BASE, flags=32), "flags = 32")
    # the index-only mode: the arrays still have D->nrows entries, though D itself meets nothing
    Dn = mat(pkg, 10, 200, None, 6)
    refused(L, pairs(L, pkg, A=A, B=B, D=Dn, ia=BASE), "overlap", "ia", "A")
    refused(L, pairs(L, pkg, A=A, B=B, D=Dn, ia=IA, wt=IA + 36), "overlap", "ia", "wt")
    if L.gf2_device_count() <= 0:
        for mname, m0 in (("A", BASE), ("B", OTHER), ("D", FAR)):
            reaches_the_device_check(L, j(ia=m0 - 40, hits=end(m0), wt=end(m0) + 16))                     # right before, right behind
        reaches_the_device_check(L, j(hits=IA - 8, ia=IA, ib=IA + 40, wt=IA + 80))                          # side by side
        reaches_the_device_check(L, j(ia=None, ib=None, wt=None))
        reaches_the_device_check(L, pairs(L, pkg, A=A, B=B, D=mat(pkg, 0, 200, None), ia=BASE, ib=BASE, wt=BASE))   # no room: empty arrays
        reaches_the_device_check(L, pairs(L, pkg, A=A, B=B, D=Dn, ia=IA, ib=IA + 40, wt=IA + 80))


# ---- arguments of gf2_nearest_dev ----------------------------------------------------------------------------------------------------------

def test_nearest_arguments(pkg, L):
    n = lambda **kw: nearest(L, pkg, **kw)  # noqa: E731
    no = lambda rc, *words: refused(L, rc, *words, entry=NEAREST)  # noqa: E731
    for name, base in (("A", BASE), ("B", OTHER)):
        no(n(**{name: None}), name + " is null")
        no(n(**{name: mat(pkg, -1, 200, base)}), name, "negative")
        no(n(**{name: mat(pkg, 10, 200, base, ld=width(200) - 1)}), name + ".ld is smaller")
        no(n(**{name: mat(pkg, 10, 200, base + 4)}), name + ".data is not 8-byte aligned")
        no(n(**{name: mat(pkg, 10, 200, None)}), name + ".data is null")
    no(n(B=mat(pkg, 12, 199, OTHER)), "must be equal")
    no(n(idx=None, dist=None), "idx and dist are both null")
    no(n(idx=IDX + 2), "idx is not 4-byte aligned")
    no(n(dist=DIST + 1), "dist is not 4-byte aligned")
    no(n(wc0=-1), "weight range", "[-1, 200)")
    no(n(wc0=101, wc1=100), "weight range")
    no(n(wc0=0, wc1=201), "weight range")
    for flags in (4, 12, -1):
        no(n(flags=flags), "flags = %d" % flags)
    no(n(flags=4, wc0=5, wc1=4), "weight range")                     # the range is reported first
    # aliasing, last: idx and dist have A->nrows entries
    A, B = mat(pkg, 10, 200, BASE, 6), mat(pkg, 12, 200, OTHER, 6)
    end = lambda at, rows: at + 8 * ((rows - 1) * 6 + width(200))   # noqa: E731
    for name in ("idx", "dist"):
        for mname, m0, rows in (("A", BASE, 10), ("B", OTHER, 12)):
            for at in (m0, m0 + 8 * 6 + 8, end(m0, rows) - 4, m0 - 36, m0 + 8 * 4):
                no(n(A=A, B=B, **{name: at}), "overlap", name, mname)
    no(n(A=A, B=B, idx=IDX, dist=IDX), "overlap", "idx", "dist")
    no(n(A=A, B=B, idx=IDX, dist=IDX + 36), "overlap", "idx", "dist")
    no(n(A=A, B=B, idx=BASE, flags=4), "flags = 4")                  # bad arguments before the overlap
    no(n(A=A, B=B, idx=BASE, dist=DIST + 2), "dist is not 4-byte aligned")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, n())
        reaches_the_device_check(L, n(idx=None))
        reaches_the_device_check(L, n(dist=None))
        for flags in (1, 2, 3):
            reaches_the_device_check(L, n(flags=flags))
        reaches_the_device_check(L, n(A=A, B=A))                      # A may be B
        reaches_the_device_check(L, n(A=A, B=mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)))
        reaches_the_device_check(L, n(wc0=0, wc1=0))
        reaches_the_device_check(L, n(wc0=200, wc1=200))
        reaches_the_device_check(L, n(A=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, n(B=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, n(A=A, B=B, idx=IDX, dist=IDX + 40))                       # side by side
        reaches_the_device_check(L, n(A=A, B=B, idx=BASE - 40, dist=end(BASE, 10)))          # right before, right behind
        reaches_the_device_check(L, n(A=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))     # rows that are only 8-byte aligned


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, na, nb, ncols, wc0, wc1):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_near_plan(na, nb, ncols, wc0, wc1, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    # the kernel follows the WORDS of a row that hold a column of the range, wherever the range lies
    ncols = 64 * 70
    expected = {0: 1, 1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8, 9: 16, 16: 16, 17: 0, 70: 0}
    for words, kernel in expected.items():
        for k0 in (0, 1, 70 - words):
            if k0 + words > 70:
                continue
            ranges = [(64 * k0, 64 * (k0 + words))]
            if words >= 2:
                ranges += [(64 * k0 + 63, 64 * (k0 + words - 1) + 1)]          # one column of the first and of the last word
            if words == 0:
                ranges = [(0, 0), (77, 77), (ncols, ncols)]
            for wc0, wc1 in ranges:
                rc, o = plan(L, 1000, 3000, ncols, wc0, wc1)
                assert rc == 0 and o[0] == kernel and o[7] == words, (words, wc0, wc1, o)
    assert plan(L, 10, 10, 256, 10, 60)[1][7] == 1                             # inside one word
    assert plan(L, 10, 10, 256, 60, 70)[1][7] == 2                             # across a word boundary
    assert plan(L, 10, 10, 256, 63, 65)[1][0::7] == [2, 2]                     # two columns, two words
    assert plan(L, 10, 10, 256, 70, 256)[1][0::7] == [4, 3]                    # 186 columns in three words: the kernel of four
    assert plan(L, 10, 10, 2000, 1, 1025)[1][0::7] == [0, 17]                  # 1024 columns that start inside a word: 17 words, wide
    assert plan(L, 10, 10, 2000, 64, 1088)[1][0::7] == [16, 16]
    for na, nb, ncols, wc in ((5, 70000, 256, (0, 256)), (700, 20000, 256, (0, 256)), (65536, 65536, 64, (0, 64)), (1 << 20, 1 << 20, 256, (70, 256)),
                              (1, 1, 1, (0, 1)), (3, 100000, 1100, (0, 1100)), (600, 600, 1025, (0, 1025)), (256, 70000, 128, (0, 128))):
        rc, (kernel, threads, rows, S, chunk, lds, scratch, words) = plan(L, na, nb, ncols, *wc)
        assert rc == 0 and threads == 256 and rows == (512 if kernel else 256) and lds == (16384 if kernel else 0) and 4 * lds <= 160 * 1024
        assert S >= 1 and S * chunk >= nb > (S - 1) * chunk and chunk <= 1 << 20           # the chunks cover B, none is empty
        assert chunk % (16384 // (8 * kernel) if kernel else 64) == 0                      # whole tiles
        assert scratch == (8 * (na * S + 1) + 15) & ~15                                    # one int64 per (row of A, chunk), and one
        assert S <= 65535                                                                    # a grid dimension
        assert device.near_plan(na, nb, ncols, wc) == (kernel, threads, rows, S, chunk, lds, scratch, words)
    # S > 1 for a small A: the chunks fill the chip
    assert plan(L, 5, 70000, 256, 0, 256)[1][3] >= 128 and plan(L, 700, 20000, 256, 0, 256)[1][3] >= 32
    assert plan(L, 1 << 20, 1 << 20, 256, 0, 256)[1][3] == 1
    # the scratch follows NA * S, not the pairs: ten times the rows of B, the same scratch
    assert plan(L, 5000, 100000, 256, 0, 256)[1][6] == plan(L, 5000, 1000000, 256, 0, 256)[1][6]
    assert plan(L, 1 << 16, 1 << 16, 256, 70, 256)[1][6] <= 16 << 20 and plan(L, 1 << 20, 1 << 20, 256, 70, 256)[1][6] <= 16 << 20
    assert device.near_plan(10, 20, 200) == device.near_plan(10, 20, 200, (0, 200))
    assert plan(L, 0, 0, 256, 0, 0)[0] == 0 and plan(L, 0, 5, 0, 0, 0)[0] == 0
    for bad in ((-1, 5, 256, 0, 9), (5, -1, 256, 0, 9), (10, 10, -1, 0, 0), (10, 10, 256, -1, 9), (10, 10, 256, 10, 9), (10, 10, 256, 0, 257),
                (10, 10, 256, 257, 257)):
        assert plan(L, *bad) == (-1, [-7] * 8), bad
        assert device.near_plan(*bad[:3], bad[3:]) is None
    assert L.gf2_near_plan(10, 10, 256, 0, 256, None) == 0 and L.gf2_near_plan(10, 10, 256, 0, 257, None) == -1
