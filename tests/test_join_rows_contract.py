"""CPU tests of the contract of include/m4ri_hip_join_rows.h (gf2_group_rows_dev, gf2_join_rows_dev, gf2_join_rows_plan): every
argument is checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around
addresses that are never dereferenced (the BASE / FAR technique of tests/test_near_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.JOIN_ROWS_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_join_rows.h")

ABASE = 1 << 20     # A, B and D: addresses that are never dereferenced
BBASE = 1 << 24
DBASE = 1 << 26
COUNT = (1 << 29) + (1 << 19)
IA = (1 << 29) + (1 << 20)
IB = (1 << 29) + (2 << 20)
WT = (1 << 29) + (3 << 20)
ORDER, HEAD = IA, IB
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

GROUP, JOIN, PLAN = "gf2_group_rows_dev", "gf2_join_rows_dev", "gf2_join_rows_plan"
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


def group(L, pkg, P=DEFAULT, c0=57, c1=200, order=ORDER, head=HEAD):
    P = mat(pkg, 10, 200) if P is DEFAULT else P
    return L.gf2_group_rows_dev(ref(P), c0, c1, order, head, None)


def join(L, pkg, D=DEFAULT, A=DEFAULT, B=DEFAULT, c0=57, c1=200, count=COUNT, ia=IA, ib=IB, wt=WT, wc0=3, wc1=190):
    D = mat(pkg, 20, 200, DBASE) if D is DEFAULT else D
    A = mat(pkg, 10, 200) if A is DEFAULT else A
    B = mat(pkg, 12, 200, BBASE) if B is DEFAULT else B
    return L.gf2_join_rows_dev(ref(D), ref(A), ref(B), c0, c1, count, ia, ib, wt, wc0, wc1, None)


def refused(L, name, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(name) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_join_rows.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_join_rows_plan(1, 1, 1, 0, 2, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {GROUP, JOIN, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.JOIN_ROWS_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS, pkg._lib.JOIN_SYMBOLS, pkg._lib.SUMS_SYMBOLS,
                  pkg._lib.JOIN_SELECT_SYMBOLS, pkg._lib.NEAR_SYMBOLS, pkg._lib.UNIQUE_SYMBOLS, pkg._lib.FIND_SYMBOLS):
        assert not declared & set(table)
    assert set(pkg._lib.FIND_SYMBOLS) == {"gf2_find_rows_dev", "gf2_find_rows_plan"}                     # ... and stay what they were
    # the argument lists are the issue's
    names = lambda decl: [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")]  # noqa: E731
    assert names(declarations()[GROUP]) == ["P", "c0", "c1", "order", "head", "stream"]
    assert names(declarations()[JOIN]) == ["D", "A", "B", "c0", "c1", "count", "ia", "ib", "wt", "wc0", "wc1", "stream"]
    assert names(declarations()[PLAN]) == ["nrows_a", "nrows_b", "ncols", "c0", "c1", "out"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("0 <= c0 <= c1 <= ncols", "c0 == c1: every value is 0", "ascending order of (rep(i), i)", "contiguous and ascending",
                  "by their lowest row", "head may be NULL", "OVERWRITTEN", "the caller zeroes nothing",
                  "exactly those of gf2_sort_rows_dev", "ceil(bits(nrows - 1) / 8) <= 4", "P->nrows == 0 writes nothing",
                  "the identity order and head all 0", "ordered by (i, j) ascending", "the order of gf2_near_pairs_dev",
                  "t < min(*count, D->nrows)", "each be NULL, independently", "a DEVICE int64", "may pass 2^31", "may pass the capacity",
                  "D->nrows == 0 is the count-only call", "the index-only mode of gf2_join_select_dev", "are not touched",
                  "by the rule of gf2_submatrix_dev", "A->ncols == B->ncols == D->ncols", "A may be B", "(i, i) included",
                  "every row meets every row", "*count = 0 and writes nothing else",
                  "(a) For c1 - c0 <= 30 the output is that of gf2_join_dev(D, A, B, c0, c1 - c0, ...) reordered by (ia, ib)",
                  "(b) For c0 == c1 the output is bit for bit that of gf2_near_pairs_dev with flags == 0, wlo = 0 and whi = ncols",
                  "(c) With A == B and i the lowest row of its class", "fixed chunks of 2048 OUTPUTS", "sized by the capacity",
                  "by bisection of the offsets", "do not depend on the order in which workgroups run", "Two calls give the same bits",
                  "no spins, flags or waits between workgroups", "Nothing outside the ncols bits of a row",
                  "only the words of a row that hold a bit of [c0, c1)", "strided views of dirty parents", "only 8-byte aligned",
                  "64-bit offsets", "Nothing of P, A and B is written", "no host synchronisation and no hipMalloc", "from a slot of its own",
                  "has been written by the same call", "before a device is required and before the first HIP call", "checked last",
                  '"overlap"', "without a device"):
        assert words in text, words


# ---- gf2_group_rows_dev -------------------------------------------------------------------------------------------------------------------

def test_group_argument_errors(pkg, L):
    no = lambda rc, *words: refused(L, GROUP, rc, *words)  # noqa: E731
    no(group(L, pkg, P=None), "P is null")
    no(group(L, pkg, mat(pkg, -1, 200)), "P", "negative")
    no(group(L, pkg, mat(pkg, 10, -200)), "P", "negative")
    no(group(L, pkg, mat(pkg, 10, 200, None)), "P.data is null")
    no(group(L, pkg, mat(pkg, 10, 200, ld=width(200) - 1)), "P.ld is smaller")
    no(group(L, pkg, mat(pkg, 10, 200, ABASE + 4)), "P.data is not 8-byte aligned")
    no(group(L, pkg, mat(pkg, 10, 200, ABASE + 4), c0=5, c1=4), "P.data is not 8-byte aligned")           # in the order of the arguments
    for c0, c1 in ((-1, 200), (0, 201), (101, 100), (201, 201), (0, -1), (1 << 30, 5)):
        no(group(L, pkg, c0=c0, c1=c1), "columns [c0, c1)", "[%d, %d)" % (c0, c1), "0 <= c0 <= c1 <= 200")
    no(group(L, pkg, order=None), "order is null")
    no(group(L, pkg, order=ORDER + 2), "order is not 4-byte aligned")
    no(group(L, pkg, head=HEAD + 1), "head is not 4-byte aligned")
    no(group(L, pkg, c0=9, c1=8, order=None), "columns [c0, c1)")
    no(group(L, pkg, order=None, head=HEAD + 1), "order is null")
    # aliasing, last
    P = mat(pkg, 10, 200, ABASE, 6)
    end = ABASE + 8 * (9 * 6 + width(200))
    for name in ("order", "head"):
        for at in (ABASE, ABASE + 8 * 6 + 8, end - 4, ABASE + 8 * 4, ABASE - 36):                           # the pad words belong to the range
            no(group(L, pkg, P, **{name: at}), "overlap", name, "P")
    no(group(L, pkg, P, order=ORDER, head=ORDER), "overlap", "order", "head")
    no(group(L, pkg, P, order=ORDER, head=ORDER + 36), "overlap", "order", "head")
    no(group(L, pkg, P, order=ABASE, head=HEAD + 2), "head is not 4-byte aligned")                          # bad arguments come first
    no(group(L, pkg, P, order=ABASE, c0=9, c1=8), "columns [c0, c1)")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, group(L, pkg))
        for c0, c1 in ((0, 0), (57, 57), (200, 200), (0, 200), (199, 200)):
            reaches_the_device_check(L, group(L, pkg, c0=c0, c1=c1))
        reaches_the_device_check(L, group(L, pkg, head=None))                                              # head may be NULL
        reaches_the_device_check(L, group(L, pkg, mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, group(L, pkg, mat(pkg, 10, 200, ABASE + 8, ld=width(200) + 1)))         # rows that are only 8-byte aligned
        reaches_the_device_check(L, group(L, pkg, P, order=ABASE - 40, head=end))                          # right before, right behind
        reaches_the_device_check(L, group(L, pkg, P, order=ORDER, head=ORDER + 40))                        # side by side


# ---- gf2_join_rows_dev --------------------------------------------------------------------------------------------------------------------

def test_join_argument_errors(pkg, L):
    no = lambda rc, *words: refused(L, JOIN, rc, *words)  # noqa: E731
    for name in ("A", "B", "D"):
        call = lambda m, **kw: join(L, pkg, **{name: m}, **kw)  # noqa: E731
        no(call(None), name + " is null")
        no(call(mat(pkg, -1, 200)), name, "negative")
        no(call(mat(pkg, 10, -200)), name, "negative")
        no(call(mat(pkg, 10, 200, ld=width(200) - 1)), name + ".ld is smaller")
        no(call(mat(pkg, 10, 200, ABASE + 4)), name + ".data is not 8-byte aligned")
        no(call(mat(pkg, 10, 200, ABASE + 4), c0=5, c1=4), name + ".data is not 8-byte aligned")          # in the order of the checks
        no(call(mat(pkg, 10, 200, ABASE + 4), count=None), name + ".data is not 8-byte aligned")
        no(call(mat(pkg, 10, 201, DBASE if name == "D" else ABASE)), "columns", "must be equal")
    no(join(L, pkg, A=mat(pkg, 10, 200, None)), "A.data is null")
    no(join(L, pkg, B=mat(pkg, 10, 200, None)), "B.data is null")
    no(join(L, pkg, A=None, B=None, D=None), "A is null")
    no(join(L, pkg, B=None, D=None), "B is null")
    for c0, c1 in ((-1, 200), (0, 201), (101, 100), (201, 201), (0, -1), (1 << 30, 5)):
        no(join(L, pkg, c0=c0, c1=c1), "columns [c0, c1)", "[%d, %d)" % (c0, c1), "0 <= c0 <= c1 <= 200")
    no(join(L, pkg, count=None), "count is null")
    no(join(L, pkg, count=COUNT + 4), "count is not 8-byte aligned")
    no(join(L, pkg, ia=IA + 2), "ia is not 4-byte aligned")
    no(join(L, pkg, ib=IB + 1), "ib is not 4-byte aligned")
    no(join(L, pkg, wt=WT + 3), "wt is not 4-byte aligned")
    for wc0, wc1 in ((-1, 5), (6, 5), (0, 201), (201, 201)):
        no(join(L, pkg, wc0=wc0, wc1=wc1), "weight range", "[%d, %d)" % (wc0, wc1), "0 <= wc0 <= wc1 <= 200")
    # in the order of the checks
    no(join(L, pkg, c0=9, c1=8, count=None), "columns [c0, c1)")
    no(join(L, pkg, count=None, ia=IA + 2), "count is null")
    no(join(L, pkg, ia=IA + 2, ib=IB + 2), "ia is not 4-byte aligned")
    no(join(L, pkg, ib=IB + 2, wt=WT + 2), "ib is not 4-byte aligned")
    no(join(L, pkg, wt=WT + 2, wc0=9, wc1=8), "wt is not 4-byte aligned")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, join(L, pkg))
        for c0, c1 in ((0, 0), (57, 57), (200, 200), (0, 200), (5, 35), (199, 200)):
            reaches_the_device_check(L, join(L, pkg, c0=c0, c1=c1))
        for wc0, wc1 in ((0, 0), (200, 200), (0, 200), (60, 70), (100, 200)):
            reaches_the_device_check(L, join(L, pkg, wc0=wc0, wc1=wc1))
        for ia, ib, wt in ((None, IB, WT), (IA, None, WT), (IA, IB, None), (None, None, None)):          # each may be NULL
            reaches_the_device_check(L, join(L, pkg, ia=ia, ib=ib, wt=wt))
        reaches_the_device_check(L, join(L, pkg, D=mat(pkg, 0, 200, None), ia=None, ib=None, wt=None))    # the count-only call
        reaches_the_device_check(L, join(L, pkg, D=mat(pkg, 20, 200, None)))                              # the index-only mode
        reaches_the_device_check(L, join(L, pkg, A=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, join(L, pkg, B=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, join(L, pkg, A=mat(pkg, 10, 200, ABASE + 8, ld=width(200) + 1)))     # rows that are only 8-byte aligned
        P = mat(pkg, 10, 200)
        reaches_the_device_check(L, join(L, pkg, A=P, B=P))                                               # A may be B
        reaches_the_device_check(L, join(L, pkg, A=P, B=mat(pkg, 4, 200, ABASE + 16, ld=4)))              # two views of one parent


def test_join_overlaps_are_refused_last(pkg, L):
    no = lambda rc, *words: refused(L, JOIN, rc, *words)  # noqa: E731
    A, B, D = mat(pkg, 10, 200, ABASE, 6), mat(pkg, 12, 200, BBASE, 7), mat(pkg, 20, 200, DBASE, 5)
    bases = {"A": ABASE, "B": BBASE, "D": DBASE}
    ends = {"A": ABASE + 8 * (9 * 6 + 4), "B": BBASE + 8 * (11 * 7 + 4), "D": DBASE + 8 * (19 * 5 + 4)}    # the first byte behind the last word
    call = lambda **kw: join(L, pkg, D=D, A=A, B=B, **kw)  # noqa: E731
    # D is written: it may share no word with A or B
    no(join(L, pkg, D=mat(pkg, 20, 200, ABASE, 6), A=A, B=B), "overlap", "D and A")
    no(join(L, pkg, D=mat(pkg, 20, 200, ABASE + 8 * 6 * 9, 6), A=A, B=B), "overlap", "D and A")
    no(join(L, pkg, D=mat(pkg, 20, 200, BBASE + 8 * 7 * 11, 7), A=A, B=B), "overlap", "D and B")
    no(join(L, pkg, D=mat(pkg, 20, 200, BBASE - 8 * 5 * 19, 5), A=A, B=B), "overlap", "D and B")          # different ld: by address range
    for m in ("A", "B", "D"):
        for name, size in (("count", 8), ("ia", 80), ("ib", 80), ("wt", 80)):
            for at in (bases[m], bases[m] + 8 * 8, ends[m] - 8, bases[m] - size + 8):
                no(call(**{name: at}), "overlap", name, m)
    no(call(ia=IA, ib=IA), "overlap", "ia", "ib")
    no(call(ia=IA, ib=IA + 76), "overlap", "ia", "ib")
    no(call(ia=IA, wt=IA - 76), "overlap", "ia", "wt")
    no(call(ib=IB, wt=IB), "overlap", "ib", "wt")
    no(call(count=IA + 72), "overlap", "count", "ia")
    no(call(count=WT), "overlap", "count", "wt")
    # bad arguments are reported before the overlap
    no(call(ia=ABASE, wt=WT + 2), "wt is not 4-byte aligned")
    no(call(ia=ABASE, wc0=9, wc1=8), "weight range")
    no(call(ia=ABASE, c0=9, c1=8), "columns [c0, c1)")
    no(join(L, pkg, D=mat(pkg, 20, 200, ABASE, 6), A=A, B=B, count=None), "count is null")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, call(ia=ABASE - 80, ib=ends["A"], wt=ends["A"] + 80, count=BBASE - 8))   # right before, right behind
        reaches_the_device_check(L, call(ia=IA, ib=IA + 80, wt=IA + 160, count=IA + 240))                   # side by side
        reaches_the_device_check(L, join(L, pkg, D=mat(pkg, 20, 200, ends["A"], 6), A=A, B=B))              # D right behind A
        reaches_the_device_check(L, join(L, pkg, D=mat(pkg, 20, 200, None, 6), A=A, B=B, ia=DBASE))         # a D without data meets nothing
        reaches_the_device_check(L, join(L, pkg, D=mat(pkg, 0, 200, ABASE, 6), A=A, B=B, ia=IA, ib=IA, wt=IA))   # no capacity: empty arrays
        reaches_the_device_check(L, join(L, pkg, D=D, A=A, B=mat(pkg, 12, 200, ABASE + 8, 6)))              # A and B may overlap


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, na, nb, ncols, c0, c1):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_join_rows_plan(na, nb, ncols, c0, c1, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    al = lambda x: (x + 15) & ~15  # noqa: E731
    for nb in (0, 1, 2, 3, 256, 257, 65536, 65537, (1 << 24) + 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 1):
        for na in (0, 7, 1 << 24):
            for ncols, c0, c1 in ((200, 57, 200), (200, 57, 57), (256, 0, 256), (1000, 3, 997), (512, 0, 512), (513, 0, 513), (577, 64, 577),
                                  (0, 0, 0)):
                passes, (slots, form, group_launches, join_launches, run_rows, chunk, group_scratch, join_scratch) = plan(L, na, nb, ncols, c0, c1)
                what = (na, nb, ncols, c0, c1)
                bits = (nb - 1).bit_length() if nb > 1 else 0
                assert passes == (bits + 7) // 8 <= 4, what                               # ceil(bits(NB - 1) / 8)
                find = device.find_rows_plan(na, nb, ncols, c0, c1)
                assert slots == find[1] and form == find[7], what                         # the table and the form of find_plan
                words = (c1 - 1) // 64 - c0 // 64 + 1 if c1 > c0 else 0
                assert form == (1 if words > 8 else 0), what
                windows = 0 if bits == 0 else 1 if bits <= 30 else 2
                sort = windows + 5 * passes if passes else 1
                assert group_launches == (3 + sort if nb else 0), what
                assert join_launches == (5 + 1 + group_launches + 1 + 1 if na and nb else 0), what
                assert (run_rows, chunk) == (1024, 2048), what
                tiles = (nb + 4095) // 4096
                work = 2 * al(8 * nb) + al(4 * 256 * tiles) + al(4 * ((256 * tiles + 2047) // 2048))
                assert group_scratch == al(12 * slots) + 2 * al(4 * nb) + work, what
                assert join_scratch == group_scratch + al(4 * nb) + 2 * al(4 * na) + al(8 * na) + al(8 * ((na + 1023) // 1024)), what
                assert device.join_rows_plan(na, nb, ncols, c0, c1) == (passes, slots, form, group_launches, join_launches, run_rows, chunk,
                                                                         group_scratch, join_scratch)
    assert [plan(L, 1, nb, 64, 0, 64)[0] for nb in (0, 1, 2, 256, 257, 65536, 65537, (1 << 24) + 1)] == [0, 0, 1, 1, 2, 2, 3, 4]
    assert device.join_rows_plan(10, 10, 200) == device.join_rows_plan(10, 10, 200, 0, 200)
    for bad in ((-1, 5, 256, 0, 9), (5, -1, 256, 0, 9), (10, 10, -1, 0, 0), (10, 10, 256, -1, 9), (10, 10, 256, 10, 9), (10, 10, 256, 0, 257),
                (10, 10, 256, 257, 257)):
        assert plan(L, *bad) == (-1, [-7] * 8), bad
        assert device.join_rows_plan(*bad) is None
    assert L.gf2_join_rows_plan(10, 10, 256, 0, 256, None) == 1 and L.gf2_join_rows_plan(10, 10, 256, 0, 257, None) == -1


# ---- the Python wrappers ----------------------------------------------------------------------------------------------------------------

def test_the_wrappers_refuse_what_the_entries_refuse(pkg, L):
    """without a device nothing can be allocated; the wrappers' own ValueErrors need none"""
    from m4ri_rust_amd import device
    A, B = device.DMat.wrap(ABASE, 10, 200, 4), device.DMat.wrap(BBASE, 12, 200, 4)
    D = device.DMat.wrap(DBASE, 20, 200, 4)
    for name in ("group_rows", "join_rows", "join_rows_plan"):
        assert callable(getattr(device, name))
    assert list(inspect.signature(device.group_rows).parameters) == ["P", "c0", "c1", "order", "head", "stream"]
    assert list(inspect.signature(device.join_rows).parameters) == ["A", "B", "c0", "c1", "D", "cap", "store", "count", "ia", "ib", "wt", "wcols",
                                                                    "stream"]
    assert list(inspect.signature(device.join_rows_plan).parameters) == ["nrows_a", "nrows_b", "ncols", "c0", "c1"]
    assert list(inspect.signature(device.DMat.group_rows).parameters) == ["self", "c0", "c1"]
    assert list(inspect.signature(device.DMat.join_rows).parameters) == ["self", "other", "c0", "c1", "wcols"]
    with pytest.raises(ValueError, match="store=False takes no D"):
        device.join_rows(A, B, D=D, store=False, count=COUNT)
    with pytest.raises(ValueError, match="a raw count address needs D or cap"):                           # the existing count-first rule
        device.join_rows(A, B, count=COUNT)
    if L.gf2_device_count() <= 0:
        with pytest.raises(pkg._lib.HipError, match="columns"):
            device.join_rows(A, B, 5, 4, D=D, count=COUNT, ia=IA, ib=IB, wt=WT)
        with pytest.raises(pkg._lib.HipError, match="weight range"):
            device.join_rows(A, B, D=D, count=COUNT, ia=IA, ib=IB, wt=WT, wcols=(5, 4))
        with pytest.raises(pkg._lib.HipError, match="no usable HIP device"):                              # c1 = None: to the last column
            device.join_rows(A, B, D=D, count=COUNT, ia=IA, ib=IB, wt=WT)
        with pytest.raises(pkg._lib.HipError, match="no usable HIP device"):                              # store=False with a capacity
            device.join_rows(A, B, cap=20, store=False, count=COUNT, ia=IA, ib=IB, wt=WT)
        with pytest.raises(pkg._lib.HipError, match="order is not 4-byte aligned"):
            device.group_rows(A, order=ORDER + 1, head=device.SKIP)
        with pytest.raises(pkg._lib.HipError, match="no usable HIP device"):
            device.group_rows(A, 3, 150, order=ORDER, head=HEAD)
