"""CPU tests of the contract of include/m4ri_hip_find.h (gf2_find_rows_dev, gf2_find_rows_plan): every argument is checked before a
device is required and before the first HIP call, so this runs without one, on DMatStructs around addresses that are never
dereferenced (the BASE / FAR technique of tests/test_near_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.FIND_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_find.h")

ABASE = 1 << 20     # A and B: addresses that are never dereferenced
BBASE = 1 << 24
IDX = (1 << 29) + (1 << 20)
MULT = (1 << 29) + (2 << 20)
COUNT = (1 << 29) + (1 << 19)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

FIND, PLAN = "gf2_find_rows_dev", "gf2_find_rows_plan"
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


def mat(pkg, nrows, ncols, data=ABASE, ld=None):
    s = pkg._lib.DMatStruct()
    s.data, s.ld, s.nrows, s.ncols = data, ld if ld is not None else (width(ncols) + 1) & ~1, nrows, ncols
    return s


def find(L, pkg, A=DEFAULT, B=DEFAULT, c0=57, c1=200, idx=IDX, mult=MULT, count=COUNT):
    A = mat(pkg, 10, 200) if A is DEFAULT else A
    B = mat(pkg, 12, 260, BBASE) if B is DEFAULT else B
    return L.gf2_find_rows_dev(ref(A), ref(B), c0, c1, idx, mult, count, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(FIND) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_find.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_find_rows_plan(1, 1, 1, 0, 2, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {FIND, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.FIND_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS, pkg._lib.JOIN_SYMBOLS, pkg._lib.SUMS_SYMBOLS,
                  pkg._lib.JOIN_SELECT_SYMBOLS, pkg._lib.NEAR_SYMBOLS, pkg._lib.UNIQUE_SYMBOLS):
        assert not declared & set(table)
    assert set(pkg._lib.UNIQUE_SYMBOLS) == {"gf2_sort_rows_dev", "gf2_unique_rows_dev", "gf2_sort_rows_plan"}   # ... and stay what they were
    # the argument lists are the issue's
    names = lambda decl: [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")]  # noqa: E731
    assert names(declarations()[FIND]) == ["A", "B", "c0", "c1", "idx", "mult", "count", "stream"]
    assert names(declarations()[PLAN]) == ["nrows_a", "nrows_b", "ncols", "c0", "c1", "out"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("0 <= c0 <= c1 <= min(A->ncols, B->ncols)", "c0 == c1: every value is 0", "the LOWEST j with value_B(j) == value_A(i)",
                  "-1 if there is none", "0 for a miss", "mult may be NULL", "count may be NULL", "OVERWRITTEN", "the caller zeroes nothing",
                  "feeds gf2_gather_rows_dev as it is", "whose compare is signed", "A may be B",
                  "bit for bit the rep of gf2_unique_rows_dev(A, c0, c1, ...)", "the size of row i's class",
                  "A->nrows == 0: *count = 0 and nothing else is written", "B->nrows == 0: idx is all -1, mult all 0, *count = 0",
                  "no table is made", "idx is all 0, mult all B->nrows and *count = A->nrows", "the lowest power of two >= 2 B->nrows",
                  "compare-and-swap", "atomic minimum", "a wave per row", "independent of the order in which workgroups run",
                  "as gf2_class_first_dev does", "an occupied slot never empties", "every class ends in exactly one slot",
                  "The layout of the table may depend on arrival order; idx, mult and count do not", "Two calls give the same bits",
                  "No thread ever waits for another", "no spins, flags or locks", "bounded by `slots`",
                  "Only the words of a row that hold a bit of [c0, c1)", "read through masks", "never influence hash or equality",
                  "never read", "strided views of dirty parents", "only 8-byte aligned", "64-bit offsets", "Nothing of A and B is written",
                  "different ncols and ld", "no host synchronisation and no hipMalloc", "from a slot of its own",
                  "has been written by the same call", "costs the caller no array", "before a device is required and before the first HIP call",
                  "in the order of the arguments", "checked last", '"overlap"', "without a device"):
        assert words in text, words


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------

def test_matrix_and_range_errors(pkg, L):
    no = lambda rc, *words: refused(L, rc, *words)  # noqa: E731
    for name, other in (("A", "B"), ("B", "A")):
        call = lambda m, **kw: find(L, pkg, **{name: m}, **kw)  # noqa: E731
        no(call(None), name + " is null")
        no(call(mat(pkg, -1, 200)), name, "negative")
        no(call(mat(pkg, 10, -200)), name, "negative")
        no(call(mat(pkg, 10, 200, None)), name + ".data is null")
        no(call(mat(pkg, 10, 200, ld=width(200) - 1)), name + ".ld is smaller")
        no(call(mat(pkg, 10, 200, ABASE + 4)), name + ".data is not 8-byte aligned")
        no(call(mat(pkg, 10, 200, ABASE + 4), c0=5, c1=4), name + ".data is not 8-byte aligned")        # in the order of the arguments
        no(call(mat(pkg, 10, 200, ABASE + 4), idx=None), name + ".data is not 8-byte aligned")
    no(find(L, pkg, A=None, B=None), "A is null")
    no(find(L, pkg, A=mat(pkg, 10, 200, ABASE + 4), B=None), "A.data is not 8-byte aligned")
    # the range against both widths: A has 200 columns, B 260
    for c0, c1 in ((-1, 200), (0, 201), (101, 100), (201, 201), (0, -1), (-2, -1), (1 << 30, 5), (0, 260)):
        no(find(L, pkg, c0=c0, c1=c1), "columns [c0, c1)", "[%d, %d)" % (c0, c1), "0 <= c0 <= c1 <= 200", "A has 200", "B 260")
    no(find(L, pkg, A=mat(pkg, 10, 300), c0=0, c1=261), "columns [c0, c1)", "0 <= c0 <= c1 <= 260", "A has 300")
    no(find(L, pkg, A=mat(pkg, 10, 300), B=mat(pkg, 5, 0, None), c0=0, c1=1), "columns [c0, c1)", "0 <= c0 <= c1 <= 0")
    no(find(L, pkg, idx=None), "idx is null")
    no(find(L, pkg, idx=IDX + 2), "idx is not 4-byte aligned")
    no(find(L, pkg, mult=MULT + 1), "mult is not 4-byte aligned")
    no(find(L, pkg, count=COUNT + 2), "count is not 4-byte aligned")
    no(find(L, pkg, idx=None, mult=MULT + 1), "idx is null")                                              # in the order of the arguments
    no(find(L, pkg, mult=MULT + 1, count=COUNT + 2), "mult is not 4-byte aligned")
    no(find(L, pkg, c0=9, c1=8, idx=None), "columns [c0, c1)")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, find(L, pkg))
        for c0, c1 in ((0, 0), (57, 57), (200, 200), (0, 200), (57, 87), (199, 200)):
            reaches_the_device_check(L, find(L, pkg, c0=c0, c1=c1))
        for mult, count in ((None, COUNT), (MULT, None), (None, None)):                                   # mult and count may be NULL
            reaches_the_device_check(L, find(L, pkg, mult=mult, count=count))
        reaches_the_device_check(L, find(L, pkg, A=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, find(L, pkg, B=mat(pkg, 0, 260, None)))
        reaches_the_device_check(L, find(L, pkg, A=mat(pkg, 10, 0, None), c0=0, c1=0))
        reaches_the_device_check(L, find(L, pkg, A=mat(pkg, 10, 200, ABASE + 8, ld=width(200) + 1)))   # rows that are only 8-byte aligned
        P = mat(pkg, 10, 200)
        reaches_the_device_check(L, find(L, pkg, A=P, B=P))                                               # A may be B
        reaches_the_device_check(L, find(L, pkg, A=P, B=mat(pkg, 4, 130, ABASE + 16, ld=4), c0=3, c1=130))   # two views of one parent


def test_an_array_inside_a_matrix_or_another_array_is_refused(pkg, L):
    A, B = mat(pkg, 10, 200, ABASE, 6), mat(pkg, 12, 260, BBASE, 7)
    ends = {"A": ABASE + 8 * (9 * 6 + width(200)), "B": BBASE + 8 * (11 * 7 + width(260))}   # the first byte behind the last word
    call = lambda **kw: find(L, pkg, A=A, B=B, **kw)  # noqa: E731
    for m, base in (("A", ABASE), ("B", BBASE)):
        places = (base, base + 8 * 6 + 8, ends[m] - 4, base + 8 * 4)                       # the pad words belong to the range
        for name, size in (("idx", 40), ("mult", 40), ("count", 4)):
            for at in places + (base - size + 4,):
                refused(L, call(**{name: at}), "overlap", name, m)
    refused(L, call(idx=IDX, mult=IDX), "overlap", "idx", "mult")
    refused(L, call(idx=IDX, mult=IDX + 36), "overlap", "idx", "mult")
    refused(L, call(idx=IDX, mult=IDX - 36), "overlap", "idx", "mult")
    refused(L, call(idx=IDX, count=IDX + 36), "overlap", "idx", "count")
    refused(L, call(mult=MULT, count=MULT), "overlap", "mult", "count")
    # bad arguments are reported before the overlap
    refused(L, call(idx=ABASE, mult=MULT + 2), "mult is not 4-byte aligned")
    refused(L, call(idx=ABASE, count=COUNT + 1), "count is not 4-byte aligned")
    refused(L, call(idx=ABASE, c0=9, c1=8), "columns [c0, c1)")
    refused(L, call(mult=BBASE, idx=None), "idx is null")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, call(idx=ABASE - 40, mult=ends["A"], count=ends["A"] + 40))       # right before, right behind
        reaches_the_device_check(L, call(idx=BBASE - 40, mult=ends["B"], count=BBASE - 44))
        reaches_the_device_check(L, call(idx=IDX, mult=IDX + 40, count=IDX + 80))                     # side by side
        reaches_the_device_check(L, call(idx=IDX, mult=None, count=None))
        reaches_the_device_check(L, find(L, pkg, A=mat(pkg, 0, 200, ABASE, 6), B=B, idx=IDX, mult=IDX, count=BBASE - 4))   # no rows of A: empty arrays
        reaches_the_device_check(L, find(L, pkg, A=A, B=mat(pkg, 0, 260, BBASE, 7), idx=BBASE))        # an empty B meets nothing


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, na, nb, ncols, c0, c1):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_find_rows_plan(na, nb, ncols, c0, c1, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    for nb in (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, (1 << 30) + 1, (1 << 31) - 1):
        for na in (0, 7, 1 << 24):
            for ncols, c0, c1 in ((200, 57, 200), (200, 57, 57), (256, 0, 256), (1000, 3, 997), (512, 0, 512), (513, 0, 513), (577, 64, 577),
                                  (0, 0, 0)):
                rc, (slots, per_slot, scratch, launches, build_rows, lookup_rows, wave, words) = plan(L, na, nb, ncols, c0, c1)
                what = (na, nb, ncols, c0, c1)
                assert rc == min(slots, (1 << 31) - 1), what
                if nb == 0:
                    assert slots == 0, what
                else:
                    assert slots >= 2 * nb and slots & (slots - 1) == 0 and (slots < 4 * nb or slots == 2), what   # the lowest such power of two
                assert per_slot == 12 and scratch == 12 * slots, what
                assert launches == (3 if na and nb else 0), what
                assert words == ((c1 - 1) // 64 - c0 // 64 + 1 if c1 > c0 else 0), what
                assert wave == (1 if words > 8 else 0) and build_rows == lookup_rows == (64 if wave else 256), what
                assert device.find_rows_plan(na, nb, ncols, c0, c1) == (rc, slots, per_slot, scratch, launches, build_rows, lookup_rows, wave, words)
    assert plan(L, 5, (1 << 30) + 1, 64, 0, 64)[1][0] == 1 << 32                                       # more than an int holds
    assert [plan(L, 1, nb, 64, 0, 64)[0] for nb in (0, 1, 2, 3, 4, 5, 1023, 1024, 1025)] == [0, 2, 4, 8, 8, 16, 2048, 2048, 4096]
    assert device.find_rows_plan(10, 10, 200) == device.find_rows_plan(10, 10, 200, 0, 200) and device.find_rows_plan(10, 10, 200)[0] == 32
    for bad in ((-1, 5, 256, 0, 9), (5, -1, 256, 0, 9), (10, 10, -1, 0, 0), (10, 10, 256, -1, 9), (10, 10, 256, 10, 9), (10, 10, 256, 0, 257),
                (10, 10, 256, 257, 257)):
        assert plan(L, *bad) == (-1, [-7] * 8), bad
        assert device.find_rows_plan(*bad) is None
    assert L.gf2_find_rows_plan(10, 10, 256, 0, 256, None) == 32 and L.gf2_find_rows_plan(10, 10, 256, 0, 257, None) == -1


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------

def test_the_wrappers_refuse_what_the_entry_refuses(pkg, L):
    """without a device nothing can be allocated; the wrappers' own ValueErrors need none"""
    from m4ri_rust_amd import device
    A = device.DMat.wrap(ABASE, 10, 200, 4)
    with pytest.raises(ValueError, match="raw idx address needs D"):
        device.gather_rows(A, IDX)
    B = device.DMat.wrap(BBASE, 12, 260, 6)
    with pytest.raises(ValueError, match="idx cannot be SKIP"):
        device.find_rows(A, B, idx=device.SKIP, mult=MULT, count=COUNT)
    for name in ("find_rows", "find_rows_plan"):
        assert callable(getattr(device, name))
    for name in ("find_in", "difference", "intersection"):
        assert callable(getattr(device.DMat, name))
    import inspect
    assert list(inspect.signature(device.find_rows).parameters) == ["A", "B", "c0", "c1", "idx", "mult", "count", "stream"]
    assert list(inspect.signature(device.find_rows_plan).parameters) == ["nrows_a", "nrows_b", "ncols", "c0", "c1"]
    for name in ("find_in", "difference", "intersection"):
        assert list(inspect.signature(getattr(device.DMat, name)).parameters) == ["self", "B", "c0", "c1"]
    if L.gf2_device_count() <= 0:
        with pytest.raises(pkg._lib.HipError, match="columns"):
            device.find_rows(A, B, 5, 4, idx=IDX, mult=device.SKIP, count=device.SKIP)
        with pytest.raises(pkg._lib.HipError, match="columns"):
            device.find_rows(A, B, 0, 201, idx=IDX, mult=device.SKIP, count=device.SKIP)
        with pytest.raises(pkg._lib.HipError, match="idx is not 4-byte aligned"):
            device.find_rows(A, B, idx=IDX + 1, mult=device.SKIP, count=device.SKIP)
        with pytest.raises(pkg._lib.HipError, match="no usable HIP device"):                           # c1 = None: the narrower of the two
            device.find_rows(A, B, idx=IDX, mult=MULT, count=COUNT)
