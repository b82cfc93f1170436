"""CPU tests of the contract of include/m4ri_hip_join.h (gf2_join_dev, gf2_join_plan): every argument is checked before a device is
required and before the first HIP call, so this runs without one, on DMatStructs around addresses that are never dereferenced (the
BASE / FAR technique of tests/test_lf2_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.JOIN_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_join.h")

BASE = 1 << 20     # A: an address that is never dereferenced
OTHER = 1 << 24    # B
FAR = 1 << 28      # D
COUNT = 1 << 29
IA = (1 << 29) + (1 << 20)
IB = (1 << 29) + (2 << 20)
WT = (1 << 29) + (3 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

JOIN, PLAN = "gf2_join_dev", "gf2_join_plan"
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


def join(L, pkg, A=DEFAULT, B=DEFAULT, D=DEFAULT, c0=37, b=20, count=COUNT, ia=IA, ib=IB, wt=WT, wc0=57, wc1=200):
    A = mat(pkg, 10, 200) if A is DEFAULT else A
    ncols = A.ncols if A is not None else 200
    B = mat(pkg, 12, ncols, OTHER) if B is DEFAULT else B
    D = mat(pkg, 10, ncols, FAR) if D is DEFAULT else D
    return L.gf2_join_dev(ref(D), ref(A), ref(B), c0, b, count, ia, ib, wt, wc0, wc1, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(JOIN) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_join.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_join_plan(1, 1, 1, 31, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {JOIN, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.JOIN_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS):   # stay what they were
        assert not declared & set(table)
    assert set(pkg._lib.LF2_SYMBOLS) == {"gf2_class_sort_dev", "gf2_lf2_reduce_dev", "gf2_lf2_plan"}
    # the argument lists are the issue's
    assert [a.split()[-1].lstrip("*") for a in declarations()[JOIN].split(",")] == ["D", "A", "B", "c0", "b", "count", "ia", "ib", "wt", "wc0",
                                                                                   "wc1", "stream"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("OVERWRITTEN", "no host synchronisation and no hipMalloc", "has been written by the same call", "never read",
                  "at most two words", "64-bit offsets", "Nothing of A or B is written", "stable class sorts", "ordered by (ia, ib)",
                  "Two runs give the same bits", "count-only call", "it may exceed 2^31", "are not touched",
                  "by the rule of gf2_submatrix_dev", "b == 0: every row has key 0", "*count = 0 and nothing else is written", "checked last",
                  '"overlap"', "before a device is required and before the first HIP call", "they may overlap or be the identical view",
                  "(i, i) included", "16-byte accesses are used only where", "without a device", "No key in common",
                  "p = l(s), ..., u(s) - 1", "independently", "0 <= wc0 <= wc1 <= ncols", "an empty range gives 0",
                  "gf2_select_weights_dev", "no atomics"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_matrix_argument_errors(pkg, L):
    j = lambda **kw: join(L, pkg, **kw)  # noqa: E731
    for name, base in (("A", BASE), ("B", OTHER), ("D", FAR)):
        refused(L, j(**{name: None}), name + " is null")
        refused(L, j(**{name: mat(pkg, 10, 200, None)}), name + ".data is null")
        refused(L, j(**{name: mat(pkg, -1, 200, base)}), name, "negative")
        refused(L, j(**{name: mat(pkg, 10, 200, base, ld=width(200) - 1)}), name + ".ld is smaller")
        refused(L, j(**{name: mat(pkg, 10, 200, base + 4)}), name + ".data is not 8-byte aligned")
    refused(L, j(A=mat(pkg, 10, -200)), "negative")
    refused(L, j(A=mat(pkg, 10, 0, None), B=mat(pkg, 3, 0, None), D=mat(pkg, 3, 0, None), c0=0, b=0, wc0=0, wc1=0), "D.data is null")   # rows without a word
    # unequal column counts, either operand
    refused(L, j(B=mat(pkg, 12, 199, OTHER)), "must be equal")
    refused(L, j(B=mat(pkg, 12, 256, OTHER)), "must be equal")
    refused(L, j(D=mat(pkg, 10, 199, FAR)), "must be equal")
    refused(L, j(D=mat(pkg, 10, 256, FAR)), "must be equal")


def test_window_count_and_array_errors(pkg, L):
    j = lambda **kw: join(L, pkg, **kw)  # noqa: E731
    for b in (-1, 31, 1 << 20):
        big = 1 << 21
        refused(L, j(A=mat(pkg, 10, big), b=b, wc1=big), "b = %d is outside 0 <= b <= 30" % b)
    refused(L, j(c0=-1), "c0", "outside A and B")
    refused(L, j(c0=181, b=20), "c0", "outside A and B")
    refused(L, j(c0=200, b=1), "c0", "outside A and B")
    refused(L, j(c0=(1 << 31) - 1, b=30), "c0", "outside A and B")
    refused(L, j(count=None), "count is null")
    refused(L, j(count=COUNT + 4), "count is not 8-byte aligned")
    refused(L, j(count=COUNT + 1), "count is not 8-byte aligned")
    refused(L, j(ia=IA + 2), "ia is not 4-byte aligned")
    refused(L, j(ib=IB + 1), "ib is not 4-byte aligned")
    refused(L, j(wt=WT + 3), "wt is not 4-byte aligned")
    # the weight range
    refused(L, j(wc0=-1), "weight range", "[-1, 200)")
    refused(L, j(wc0=101, wc1=100), "weight range")
    refused(L, j(wc0=0, wc1=201), "weight range")
    refused(L, j(wc0=201, wc1=201), "weight range")
    refused(L, j(wc0=0, wc1=-1), "weight range")
    refused(L, j(wt=None, wc0=5, wc1=4), "weight range")           # also where no weight is asked for
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, j())
        for skipped in ({"ia": None}, {"ib": None}, {"wt": None}, {"ia": None, "wt": None}, {"ia": None, "ib": None, "wt": None}):
            reaches_the_device_check(L, j(**skipped))
        reaches_the_device_check(L, j(wc0=0, wc1=0))                  # empty ranges
        reaches_the_device_check(L, j(wc0=200, wc1=200))
        reaches_the_device_check(L, j(wc0=0, wc1=200))                # the whole row, the window included
        reaches_the_device_check(L, j(c0=180, b=20))                  # up to the last column
        reaches_the_device_check(L, j(c0=50, b=30))                   # over a word boundary
        reaches_the_device_check(L, j(c0=200, b=0))                   # no window bit at all
        reaches_the_device_check(L, j(D=mat(pkg, 0, 200, None)))      # the count-only form
        reaches_the_device_check(L, j(D=mat(pkg, 0, 200, None), ia=None, ib=None, wt=None))
        reaches_the_device_check(L, j(A=mat(pkg, 0, 200, None)))      # no row on either side
        reaches_the_device_check(L, j(B=mat(pkg, 0, 200, None)))
        # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
        reaches_the_device_check(L, j(A=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, j(B=mat(pkg, 12, 200, OTHER + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, j(D=mat(pkg, 10, 200, FAR + 8, ld=width(200) + 1)))


def test_a_and_b_may_overlap_or_be_one_view(pkg, L):
    A = mat(pkg, 10, 200, BASE, 6)
    j = lambda B, **kw: join(L, pkg, A=A, B=B, c0=0, b=4, **kw)  # noqa: E731
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, j(A))                                              # the identical view: a self-join
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE, 6)))                     # the same words under another struct
        reaches_the_device_check(L, j(mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)))          # some of A's rows
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE + 8 * 3, 6)))             # shifted by three words
        reaches_the_device_check(L, j(mat(pkg, 10, 200, BASE + 8, 8)))                 # another ld
    refused(L, j(A, D=mat(pkg, 10, 200, BASE, 6)), "overlap", "D", "A")               # ... but D may not be one of them


def test_d_may_share_no_word_with_a_or_b(pkg, L):
    for name, base in (("A", BASE), ("B", OTHER)):
        M = mat(pkg, 10, 200, base, 6)
        j = lambda D, M=M, name=name, **kw: join(L, pkg, D=D, c0=0, b=4, **{name: M}, **kw)  # noqa: E731
        refused(L, j(mat(pkg, 10, 200, base, 6)), "overlap", "D", name)                      # in place
        refused(L, j(mat(pkg, 5, 200, base + 8 * 6 * 3, 6)), "overlap", "D", name)           # some of its rows
        refused(L, j(mat(pkg, 10, 200, base + 8 * 3, 6)), "overlap", "D", name)              # shifted by three words: shares one
        refused(L, j(mat(pkg, 10, 200, base - 8 * 6 * 9, 6)), "overlap", "D", name)          # its last row is the operand's first
        refused(L, j(mat(pkg, 10, 200, base + 8, 8)), "overlap", "D", name)                  # another ld: address ranges
        refused(L, j(mat(pkg, 10, 200, base, 6), count=COUNT + 4), "count is not 8-byte aligned")   # bad arguments first
        refused(L, j(mat(pkg, 10, 200, base, 6), wc0=9, wc1=8), "weight range")
        if L.gf2_device_count() <= 0:
            reaches_the_device_check(L, j(mat(pkg, 10, 200, base + 8 * 6 * 10, 6)))          # right behind
            reaches_the_device_check(L, j(mat(pkg, 10, 200, base - 8 * 6 * 10, 6)))          # right before
            reaches_the_device_check(L, j(mat(pkg, 0, 200, None)))                           # no room: D is empty


def test_an_array_inside_an_operand_is_refused(pkg, L):
    A = mat(pkg, 10, 200, BASE, 6)
    B = mat(pkg, 10, 200, OTHER, 6)
    D = mat(pkg, 10, 200, FAR, 6)
    end = lambda at: at + 8 * (9 * 6 + width(200))   # noqa: E731  the first byte behind the last word of a 10 x 200, ld 6
    j = lambda **kw: join(L, pkg, A=A, B=B, D=D, c0=0, b=4, **kw)  # noqa: E731
    for name, size, step in (("count", 8, 8), ("ia", 40, 4), ("ib", 40, 4), ("wt", 40, 4)):
        for mname, m0 in (("A", BASE), ("B", OTHER), ("D", FAR)):
            for at in (m0, m0 + 8 * 6 + 8, end(m0) - step, m0 - size + step, m0 + 8 * 4):   # the pad words belong to the range
                refused(L, j(**{name: at}), "overlap", name, mname)
    # ... and against each other
    refused(L, j(count=IA, ia=IA), "overlap", "count", "ia")
    refused(L, j(count=IA + 32, ia=IA), "overlap", "count", "ia")
    refused(L, j(count=IB + 32, ib=IB), "overlap", "count", "ib")
    refused(L, j(count=WT + 32, wt=WT), "overlap", "count", "wt")
    refused(L, j(ia=IA, ib=IA), "overlap", "ia", "ib")
    refused(L, j(ia=IA, ib=IA + 36), "overlap", "ia", "ib")
    refused(L, j(ia=IA, wt=IA - 36), "overlap", "ia", "wt")
    refused(L, j(ib=IB, wt=IB + 4), "overlap", "ib", "wt")
    # bad arguments are reported before the overlap
    refused(L, join(L, pkg, A=A, B=B, D=D, c0=0, b=31, count=BASE), "b = 31")
    refused(L, j(ia=BASE, count=None), "count is null")
    refused(L, j(ia=BASE, wt=WT + 2), "wt is not 4-byte aligned")
    refused(L, j(ia=BASE, wc0=300, wc1=300), "weight range")
    if L.gf2_device_count() <= 0:
        for mname, m0 in (("A", BASE), ("B", OTHER), ("D", FAR)):
            reaches_the_device_check(L, j(ia=m0 - 40, count=end(m0), wt=end(m0) + 8))        # right before, right behind
        reaches_the_device_check(L, j(count=IA - 8, ia=IA, ib=IA + 40, wt=IA + 80))          # side by side
        reaches_the_device_check(L, j(ia=None, ib=None, wt=None))                            # a null array meets nothing
        reaches_the_device_check(L, join(L, pkg, A=A, B=B, D=mat(pkg, 0, 200, None), c0=0, b=4, ia=BASE, ib=BASE, wt=BASE))   # no room: empty arrays


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, na, nb, ncols, b):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_join_plan(na, nb, ncols, b, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    assert [plan(L, 1000, 3000, 256, b)[0] for b in (0, 1, 8, 9, 30)] == [0, 1, 1, 2, 4]
    na, nb = 100003, 40007
    lanes_by_width = []
    for words in (1, 2, 3, 4, 5, 64, 65):
        ncols = 64 * words - 3
        seen = set()
        for b in (0, 1, 8, 9, 30):
            passes, o = plan(L, na, nb, ncols, b)
            threads, R, lanes, S, lds, scratch, runs, sort_bytes = o
            assert passes == -(-b // 8), (b, o)
            assert threads in (64, 128, 256, 512, 1024) and R >= threads and R % threads == 0 and S >= 1, (b, o)
            assert lds >= 8 * R + 4 * R + 4 * S and 2 * lds <= 160 * 1024, (b, o)        # two workgroups per CU at the least
            assert lanes in (1, 2, 8, 64) and lanes == device.lf2_plan(na, ncols, b)[6], (b, o)   # the thresholds of the LF2 pair scatter
            assert runs == -(-na // R), (b, o)
            assert sort_bytes == (max(device.lf2_plan(n, ncols, b)[7] for n in (na, nb)) if b else 0), (b, o)
            assert scratch >= sort_bytes + 8 * na + 8 * nb + 8 * runs, (b, o)           # ... order and keys of A and B, run sums
            assert device.join_plan(na, nb, ncols, b) == (passes,) + tuple(o)
            seen.add((threads, R, lanes, S, lds, runs))
        assert len(seen) == 1                                # all but the passes and the sort's space follow the shape alone
        lanes_by_width.append(lanes)
    assert lanes_by_width == sorted(lanes_by_width) and lanes_by_width[0] == 1     # wider rows never get fewer lanes
    assert lanes_by_width[2] == lanes_by_width[3] and lanes_by_width[4] == lanes_by_width[5] < lanes_by_width[6]
    assert plan(L, 0, 0, 256, 8)[0] == 1 and plan(L, 0, 5, 0, 0)[0] == 0
    for bad in ((-1, 5, 256, 8), (5, -1, 256, 8), (10, 10, -1, 8), (10, 10, 256, -1), (10, 10, 256, 31)):
        assert plan(L, *bad) == (-1, [-7] * 8)
        assert device.join_plan(*bad) is None
    assert L.gf2_join_plan(10, 10, 256, 20, None) == 3 and L.gf2_join_plan(10, 10, 256, 31, None) == -1
