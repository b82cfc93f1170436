"""CPU tests of the contract of include/m4ri_hip_unique.h (gf2_sort_rows_dev, gf2_unique_rows_dev, gf2_sort_rows_plan): every argument
is checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around addresses that
are never dereferenced (the BASE / FAR technique of tests/test_near_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.UNIQUE_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_unique.h")

BASE = 1 << 20     # P: an address that is never dereferenced
ORDER = (1 << 29) + (1 << 20)
HEAD = (1 << 29) + (2 << 20)
KEEP, COUNT, REP = ORDER, (1 << 29) + (1 << 19), HEAD
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

SORT, UNIQUE, PLAN = "gf2_sort_rows_dev", "gf2_unique_rows_dev", "gf2_sort_rows_plan"
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


def sort(L, pkg, P=DEFAULT, c0=57, c1=200, order=ORDER, head=HEAD):
    P = mat(pkg, 10, 200) if P is DEFAULT else P
    return L.gf2_sort_rows_dev(ref(P), c0, c1, order, head, None)


def unique(L, pkg, P=DEFAULT, c0=57, c1=200, keep=KEEP, cap=10, count=COUNT, rep=REP):
    P = mat(pkg, 10, 200) if P is DEFAULT else P
    return L.gf2_unique_rows_dev(ref(P), c0, c1, keep, cap, count, rep, None)


def refused(L, rc, *words, entry=SORT):
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
    src.write_text('#include "m4ri_hip_unique.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_sort_rows_plan(1, 1, 0, 2, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {SORT, UNIQUE, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.UNIQUE_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS, pkg._lib.DRAW_SYMBOLS, pkg._lib.JOIN_SYMBOLS, pkg._lib.SUMS_SYMBOLS,
                  pkg._lib.JOIN_SELECT_SYMBOLS, pkg._lib.NEAR_SYMBOLS):
        assert not declared & set(table)
    assert set(pkg._lib.NEAR_SYMBOLS) == {"gf2_near_pairs_dev", "gf2_nearest_dev", "gf2_near_plan"}        # ... and stay what they were
    assert set(pkg._lib.LF2_SYMBOLS) == {"gf2_class_sort_dev", "gf2_lf2_reduce_dev", "gf2_lf2_plan"}
    # the argument lists are the issue's
    names = lambda decl: [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")]  # noqa: E731
    assert names(declarations()[SORT]) == ["P", "c0", "c1", "order", "head", "stream"]
    assert names(declarations()[UNIQUE]) == ["P", "c0", "c1", "keep", "cap", "count", "rep", "stream"]
    assert names(declarations()[PLAN]) == ["nrows", "ncols", "c0", "c1", "out"]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("column c1 - 1 is the most significant bit", "0 <= c0 <= c1 <= P->ncols", "c0 == c1: every value is 0",
                  "ascending by (value, row index)", "STABLE sort", "the result is unique", "head[s] <= s and head[head[s]] == head[s]",
                  "gf2_class_sort_dev(P, c0, c1 - c0, order, NULL, stream)", "bit for bit", "KEPT iff no row j < i has value(j) == value(i)",
                  "t < min(*count, cap)", "entries behind that are not touched", "it may exceed cap", "keep may be NULL iff cap == 0",
                  "rep[i] == i iff row i is kept", "OVERWRITTEN", "feeds gf2_gather_rows_dev as it is", "gather as zero",
                  "nrows == 0: *count = 0 and nothing else is written", "gf2_sort_rows_dev writes nothing", "order is the identity",
                  "head is all 0", "*count = 1", "rep is all 0", "windows of 24 columns", "least significant first",
                  "ceil((c1 - c0) / 8) passes", "No atomics are used", "one writer per output word", "Two runs give the same bits",
                  "Only the words of a row that hold a bit of [c0, c1)", "read through masks", "never influence a result", "never read",
                  "strided view of a dirty parent", "16-byte accesses are used only where", "64-bit offsets", "Nothing of P is written",
                  "no host synchronisation and no hipMalloc", "from a slot of its own", "has been written by the same call",
                  "costs the caller no array", "before a device is required and before the first HIP call", "in the order of the arguments",
                  "checked last", '"overlap"', "without a device"):
        assert words in text, words


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------

def both(L, pkg):
    return ((SORT, lambda **kw: sort(L, pkg, **kw)), (UNIQUE, lambda **kw: unique(L, pkg, **kw)))


def test_matrix_and_range_errors(pkg, L):
    for entry, call in both(L, pkg):
        no = lambda rc, *words: refused(L, rc, *words, entry=entry)  # noqa: E731
        no(call(P=None), "P is null")
        no(call(P=mat(pkg, -1, 200)), "P", "negative")
        no(call(P=mat(pkg, 10, -200)), "P", "negative")
        no(call(P=mat(pkg, 10, 200, None)), "P.data is null")
        no(call(P=mat(pkg, 10, 200, ld=width(200) - 1)), "P.ld is smaller")
        no(call(P=mat(pkg, 10, 200, BASE + 4)), "P.data is not 8-byte aligned")
        for c0, c1 in ((-1, 200), (0, 201), (101, 100), (201, 201), (0, -1), (-2, -1), (1 << 30, 5)):
            no(call(c0=c0, c1=c1), "columns [c0, c1)", "[%d, %d)" % (c0, c1), "0 <= c0 <= c1 <= 200")
        no(call(P=mat(pkg, 10, 200, BASE + 4), c0=5, c1=4), "P.data is not 8-byte aligned")            # in the order of the arguments
    no = lambda rc, *words: refused(L, rc, *words, entry=SORT)  # noqa: E731
    no(sort(L, pkg, order=None), "order is null")
    no(sort(L, pkg, order=ORDER + 2), "order is not 4-byte aligned")
    no(sort(L, pkg, head=HEAD + 1), "head is not 4-byte aligned")
    no(sort(L, pkg, order=None, head=HEAD + 1), "order is null")
    no(sort(L, pkg, c0=9, c1=8, order=None), "columns [c0, c1)")
    no = lambda rc, *words: refused(L, rc, *words, entry=UNIQUE)  # noqa: E731
    no(unique(L, pkg, count=None), "count is null")
    no(unique(L, pkg, count=COUNT + 2), "count is not 4-byte aligned")
    no(unique(L, pkg, keep=None), "keep is null")                       # cap > 0
    no(unique(L, pkg, keep=None, cap=1), "keep is null")
    no(unique(L, pkg, keep=KEEP + 3), "keep is not 4-byte aligned")
    no(unique(L, pkg, cap=-1), "cap = -1 is negative")
    no(unique(L, pkg, keep=None, cap=-5), "cap = -5 is negative")
    no(unique(L, pkg, rep=REP + 2), "rep is not 4-byte aligned")
    no(unique(L, pkg, keep=None, count=None), "keep is null")           # in the order of the arguments
    no(unique(L, pkg, count=None, rep=REP + 2), "count is null")
    no(unique(L, pkg, c0=201, c1=201, keep=None), "columns [c0, c1)")
    if L.gf2_device_count() <= 0:
        for entry, call in both(L, pkg):
            reaches_the_device_check(L, call())
            for c0, c1 in ((0, 0), (57, 57), (200, 200), (0, 200), (57, 87), (57, 88), (199, 200)):
                reaches_the_device_check(L, call(c0=c0, c1=c1))
            reaches_the_device_check(L, call(P=mat(pkg, 0, 200, None)))
            reaches_the_device_check(L, call(P=mat(pkg, 10, 0, None), c0=0, c1=0))
            reaches_the_device_check(L, call(P=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))     # rows that are only 8-byte aligned
        reaches_the_device_check(L, sort(L, pkg, head=None))
        reaches_the_device_check(L, unique(L, pkg, rep=None))
        reaches_the_device_check(L, unique(L, pkg, keep=None, cap=0))                                # the count-only call
        reaches_the_device_check(L, unique(L, pkg, keep=None, cap=0, rep=None))
        reaches_the_device_check(L, unique(L, pkg, cap=0))
        reaches_the_device_check(L, unique(L, pkg, cap=1))
        reaches_the_device_check(L, unique(L, pkg, cap=(1 << 31) - 1, keep=1 << 40, count=COUNT, rep=REP))


def test_an_array_inside_p_or_another_array_is_refused(pkg, L):
    P = mat(pkg, 10, 200, BASE, 6)
    end = BASE + 8 * (9 * 6 + width(200))            # the first byte behind the last word of a 10 x 200, ld 6
    places = (BASE, BASE + 8 * 6 + 8, end - 4, BASE + 8 * 4)                 # the pad words belong to the range
    for name in ("order", "head"):
        for at in places + (BASE - 36,):
            refused(L, sort(L, pkg, P=P, **{name: at}), "overlap", name, "P")
    refused(L, sort(L, pkg, P=P, order=ORDER, head=ORDER), "overlap", "order", "head")
    refused(L, sort(L, pkg, P=P, order=ORDER, head=ORDER + 36), "overlap", "order", "head")
    refused(L, sort(L, pkg, P=P, order=ORDER, head=ORDER - 36), "overlap", "order", "head")
    # bad arguments are reported before the overlap
    refused(L, sort(L, pkg, P=P, order=BASE, head=HEAD + 2), "head is not 4-byte aligned")
    refused(L, sort(L, pkg, P=P, order=BASE, c0=9, c1=8), "columns [c0, c1)")
    no = lambda rc, *words: refused(L, rc, *words, entry=UNIQUE)  # noqa: E731
    for name, size in (("keep", 40), ("count", 4), ("rep", 40)):
        for at in places + (BASE - size + 4,):
            no(unique(L, pkg, P=P, **{name: at}), "overlap", name, "P")
    no(unique(L, pkg, P=P, keep=KEEP, count=KEEP + 36), "overlap", "keep", "count")
    no(unique(L, pkg, P=P, keep=KEEP, rep=KEEP + 36), "overlap", "keep", "rep")
    no(unique(L, pkg, P=P, keep=KEEP, cap=3, rep=KEEP + 8), "overlap", "keep", "rep")
    no(unique(L, pkg, P=P, count=REP + 20, rep=REP), "overlap", "count", "rep")
    no(unique(L, pkg, P=P, keep=BASE, count=None), "count is null")
    no(unique(L, pkg, P=P, keep=BASE, rep=REP + 1), "rep is not 4-byte aligned")
    no(unique(L, pkg, P=P, rep=BASE, cap=-1), "cap = -1 is negative")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, sort(L, pkg, P=P, order=BASE - 40, head=end))                    # right before, right behind
        reaches_the_device_check(L, sort(L, pkg, P=P, order=ORDER, head=ORDER + 40))                 # side by side
        reaches_the_device_check(L, unique(L, pkg, P=P, keep=BASE - 40, count=end, rep=end + 4))
        reaches_the_device_check(L, unique(L, pkg, P=P, keep=KEEP, cap=3, rep=KEEP + 12, count=KEEP + 52))
        reaches_the_device_check(L, unique(L, pkg, P=P, keep=BASE, cap=0))                           # no room: an empty array
        reaches_the_device_check(L, unique(L, pkg, P=mat(pkg, 0, 200, BASE, 6), rep=BASE, keep=KEEP))   # an empty P meets nothing


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, nrows, ncols, c0, c1):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_sort_rows_plan(nrows, ncols, c0, c1, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    for nrows, ncols, c0, c1 in ((1000, 200, 57, 200), (1000, 200, 57, 57), (1, 1, 0, 1), (5, 64, 0, 64), (4097, 200, 57, 87), (4097, 200, 57, 88),
                                 (1 << 20, 256, 0, 256), (1 << 24, 256, 0, 24), (3 * 4096 + 5, 1000, 3, 997), (0, 256, 0, 256), (0, 0, 0, 0),
                                 (77, 257, 63, 257), (77, 300, 10, 10 + 24), (77, 300, 10, 10 + 25), (77, 300, 10, 10 + 48)):
        rc, (windows, bits, passes, sort_launches, unique_launches, sort_scratch, unique_scratch, run) = plan(L, nrows, ncols, c0, c1)
        b = c1 - c0
        assert rc == passes == (b + 7) // 8, (nrows, ncols, c0, c1)               # as many as one sort of a key that wide would take
        assert bits == 24 and windows == (b + 23) // 24 and run == 1024
        assert sort_launches == (windows + 5 * passes if b else 1) and unique_launches == sort_launches + 7
        tiles, runs = (nrows + 4095) // 4096, (nrows + 1023) // 1024
        a16 = lambda x: (x + 15) & ~15  # noqa: E731
        work = 2 * a16(8 * nrows) + a16(4 * 256 * tiles) + a16(4 * ((256 * tiles + 2047) // 2048))
        assert sort_scratch == work + a16(4 * runs)
        assert unique_scratch == sort_scratch + a16(4 * nrows) + a16(4 * ((nrows + 1023) // 1024))
        assert device.sort_rows_plan(nrows, ncols, c0, c1) == (rc, windows, bits, passes, sort_launches, unique_launches, sort_scratch,
                                                                unique_scratch, run)
    assert device.sort_rows_plan(10, 200) == device.sort_rows_plan(10, 200, 0, 200) and device.sort_rows_plan(10, 200)[0] == 25
    lf2 = device.lf2_plan(1 << 20, 256, 24)
    assert plan(L, 1 << 20, 256, 0, 24)[0] == lf2[0] and plan(L, 1 << 20, 256, 0, 24)[1][5] >= lf2[7]   # the passes and work of the class sort
    for bad in ((-1, 256, 0, 9), (10, -1, 0, 0), (10, 256, -1, 9), (10, 256, 10, 9), (10, 256, 0, 257), (10, 256, 257, 257)):
        assert plan(L, *bad) == (-1, [-7] * 8), bad
        assert device.sort_rows_plan(*bad) is None
    assert L.gf2_sort_rows_plan(10, 256, 0, 256, None) == 32 and L.gf2_sort_rows_plan(10, 256, 0, 257, None) == -1
