"""CPU tests of the contract of include/m4ri_hip_lf2.h (gf2_class_sort_dev, gf2_lf2_reduce_dev, gf2_lf2_plan): every argument is
checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around addresses that are
never dereferenced (the BASE / FAR technique of tests/test_bkw_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.LF2_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_lf2.h")

BASE = 1 << 20     # P: an address that is never dereferenced
FAR = 1 << 28      # D
COUNT = 1 << 29
LO = (1 << 29) + (1 << 20)
HI = (1 << 29) + (2 << 20)
ORDER = 1 << 30
SKEYS = (1 << 30) + (1 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

SORT, REDUCE, PLAN = "gf2_class_sort_dev", "gf2_lf2_reduce_dev", "gf2_lf2_plan"
ENTRIES = (SORT, REDUCE)


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


DEFAULT = object()


def sort(L, P, c0=37, b=20, order=ORDER, skeys=SKEYS):
    return L.gf2_class_sort_dev(ref(P), c0, b, order, skeys, None)


def reduce(L, pkg, P, D=DEFAULT, c0=37, b=20, count=COUNT, lo=LO, hi=HI):
    if D is DEFAULT:
        D = mat(pkg, 10, P.ncols if P is not None else 200, FAR)
    return L.gf2_lf2_reduce_dev(ref(D), ref(P), c0, b, count, lo, hi, None)


def call(L, pkg, name, P, **kw):
    return sort(L, P, **kw) if name == SORT else reduce(L, pkg, P, **kw)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_lf2.h"\nint main(void){ gf2_dmat d; long long o[8]; (void)d; '
                   'return gf2_lf2_plan(1, 1, 31, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {SORT, REDUCE, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.LF2_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS):   # stay what they were
        assert not declared & set(table)
    assert set(pkg._lib.BKW_SYMBOLS) == {"gf2_class_first_dev", "gf2_lf1_reduce_dev", "gf2_lf1_plan"}


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("OVERWRITTEN", "no host synchronisation and no hipMalloc", "has been written by the same call", "never read",
                  "at most two words", "64-bit offsets", "Nothing of P is written", "STABLE sort", "ties come in ascending row order",
                  "Two runs give the same bits", "ordered by (hi, lo)", "count-only call", "it may exceed 2^31", "are not touched",
                  "by the rule of gf2_submatrix_dev", "b == 0: every row has key 0", "nrows == 0: *count = 0", "checked last",
                  '"overlap"', "before a device is required and before the first HIP call", "no in-place round",
                  "16-byte accesses are used only where", "without a device", "All keys distinct", "p = t(s), ..., s - 1",
                  "skeys may be NULL", "independently"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ENTRIES)
def test_argument_errors(pkg, L, name):
    P = mat(pkg, 10, 200)
    c = lambda P, **kw: call(L, pkg, name, P, **kw)  # noqa: E731
    refused(L, c(None), name, "P is null")
    refused(L, c(mat(pkg, 10, 200, None)), name, "P.data is null")
    refused(L, c(mat(pkg, -1, 200)), name, "negative")
    refused(L, c(mat(pkg, 10, -200)), name, "negative")
    refused(L, c(mat(pkg, 10, 200, ld=width(200) - 1)), name, "P.ld is smaller")
    refused(L, c(mat(pkg, 10, 200, BASE + 4)), name, "P.data is not 8-byte aligned")
    for b in (-1, 31, 1 << 20):
        refused(L, c(mat(pkg, 10, 1 << 21), b=b), name, "b = %d is outside 0 <= b <= 30" % b)
    refused(L, c(P, c0=-1), name, "c0", "outside P")
    refused(L, c(P, c0=181, b=20), name, "c0", "outside P")
    refused(L, c(P, c0=200, b=1), name, "c0", "outside P")
    refused(L, c(P, c0=(1 << 31) - 1, b=30), name, "c0", "outside P")
    assert L.gf2_last_error().decode().startswith(name)
    if L.gf2_device_count() <= 0:
        # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
        reaches_the_device_check(L, c(mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, c(P, c0=180, b=20))     # up to the last column
        reaches_the_device_check(L, c(P, c0=50, b=30))      # over a word boundary
        reaches_the_device_check(L, c(P, c0=200, b=0))      # no window bit at all
        reaches_the_device_check(L, c(P, c0=0, b=0))
        reaches_the_device_check(L, c(mat(pkg, 0, 200, None)))   # no row
        reaches_the_device_check(L, c(mat(pkg, 7, 0, None), c0=0, b=0))


def test_sort_argument_errors(pkg, L):
    P = mat(pkg, 10, 200)
    refused(L, sort(L, P, order=None), SORT, "order is null")
    refused(L, sort(L, P, order=ORDER + 2), SORT, "order is not 4-byte aligned")
    refused(L, sort(L, P, skeys=SKEYS + 1), SORT, "skeys is not 4-byte aligned")
    assert L.gf2_last_error().decode().startswith(SORT)
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, sort(L, P))
        reaches_the_device_check(L, sort(L, P, skeys=None))
        reaches_the_device_check(L, sort(L, P, order=ORDER + 4, skeys=None))
        reaches_the_device_check(L, sort(L, P, c0=0, b=0, skeys=None))


def test_reduce_argument_errors(pkg, L):
    P = mat(pkg, 10, 200)
    r = lambda P=P, **kw: reduce(L, pkg, P, **kw)  # noqa: E731
    refused(L, r(D=None), REDUCE, "D is null")
    refused(L, r(D=mat(pkg, 10, 200, None)), REDUCE, "D.data is null")
    refused(L, r(P=mat(pkg, 10, 0, None), D=mat(pkg, 3, 0, None), c0=0, b=0), REDUCE, "D.data is null")   # rows without a word
    refused(L, r(D=mat(pkg, -1, 200, FAR)), REDUCE, "negative")
    refused(L, r(D=mat(pkg, 10, 200, FAR, ld=width(200) - 1)), REDUCE, "D.ld is smaller")
    refused(L, r(D=mat(pkg, 10, 200, FAR + 4)), REDUCE, "D.data is not 8-byte aligned")
    refused(L, r(count=None), REDUCE, "count is null")
    refused(L, r(count=COUNT + 4), REDUCE, "count is not 8-byte aligned")
    refused(L, r(count=COUNT + 1), REDUCE, "count is not 8-byte aligned")
    refused(L, r(lo=LO + 2), REDUCE, "lo is not 4-byte aligned")
    refused(L, r(hi=HI + 1), REDUCE, "hi is not 4-byte aligned")
    refused(L, r(D=mat(pkg, 10, 199, FAR)), REDUCE, "D->ncols must equal P->ncols")
    refused(L, r(D=mat(pkg, 10, 256, FAR)), REDUCE, "D->ncols must equal P->ncols")
    assert L.gf2_last_error().decode().startswith(REDUCE)
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, r())
        reaches_the_device_check(L, r(lo=None))
        reaches_the_device_check(L, r(hi=None))
        reaches_the_device_check(L, r(lo=None, hi=None))
        reaches_the_device_check(L, r(D=mat(pkg, 0, 200, None)))                    # the count-only form
        reaches_the_device_check(L, r(D=mat(pkg, 0, 200, None), lo=None, hi=None))
        reaches_the_device_check(L, r(D=mat(pkg, 1000, 200, FAR)))
        reaches_the_device_check(L, r(D=mat(pkg, 10, 200, FAR + 8, ld=width(200) + 1)))   # odd ld at an odd word, D ...
        reaches_the_device_check(L, r(P=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))  # ... and P
        reaches_the_device_check(L, r(P=mat(pkg, 0, 200, None), D=mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, r(c0=0, b=0))


def test_an_array_inside_an_operand_is_refused(pkg, L):
    P = mat(pkg, 10, 200, BASE, 6)
    D = mat(pkg, 10, 200, FAR, 6)
    b = 4
    end = lambda at: at + 8 * (9 * 6 + width(200))   # noqa: E731  the first byte behind the last word of a 10 x 200, ld 6
    # the sort: order and skeys hold P->nrows ints each
    for name in ("order", "skeys"):
        for at in (BASE, BASE + 8 * 6 + 8, end(BASE) - 4, BASE - 40 + 4, BASE + 8 * 4):   # the pad words belong to the range
            refused(L, sort(L, P, c0=0, b=b, **{name: at}), SORT, "overlap", name, "P")
    refused(L, sort(L, P, c0=0, b=b, order=ORDER, skeys=ORDER), SORT, "overlap", "order", "skeys")
    refused(L, sort(L, P, c0=0, b=b, order=ORDER, skeys=ORDER + 36), SORT, "overlap", "order", "skeys")
    refused(L, sort(L, P, c0=0, b=b, order=ORDER, skeys=ORDER - 36), SORT, "overlap", "order", "skeys")
    refused(L, sort(L, P, c0=0, b=31, order=BASE), SORT, "b = 31")            # bad arguments before the overlap
    refused(L, sort(L, P, c0=190, b=20, order=BASE), SORT, "outside P")
    refused(L, sort(L, P, c0=0, b=b, order=BASE, skeys=SKEYS + 2), SORT, "skeys is not 4-byte aligned")
    # the reduction: every array against both matrices
    r = lambda **kw: reduce(L, pkg, P, D=D, c0=0, b=b, **kw)  # noqa: E731
    for name, size, step in (("count", 8, 8), ("lo", 40, 4), ("hi", 40, 4)):
        for mname, m0 in (("P", BASE), ("D", FAR)):
            for at in (m0, m0 + 8 * 6 + 8, end(m0) - step, m0 - size + step, m0 + 8 * 4):
                refused(L, r(**{name: at}), REDUCE, "overlap", name, mname)
    # ... and against each other
    refused(L, r(count=LO, lo=LO), REDUCE, "overlap", "count", "lo")
    refused(L, r(count=LO + 32, lo=LO), REDUCE, "overlap", "count", "lo")
    refused(L, r(count=HI + 32, hi=HI), REDUCE, "overlap", "count", "hi")
    refused(L, r(lo=LO, hi=LO), REDUCE, "overlap", "lo", "hi")
    refused(L, r(lo=LO, hi=LO + 36), REDUCE, "overlap", "lo", "hi")
    refused(L, r(lo=LO, hi=LO - 36), REDUCE, "overlap", "lo", "hi")
    # bad arguments are reported before the overlap
    refused(L, reduce(L, pkg, P, D=D, c0=0, b=31, count=BASE), REDUCE, "b = 31")
    refused(L, r(lo=BASE, count=None), REDUCE, "count is null")
    refused(L, r(lo=BASE, hi=HI + 2), REDUCE, "hi is not 4-byte aligned")
    refused(L, reduce(L, pkg, P, D=mat(pkg, 10, 201, BASE, 6), c0=0, b=b), REDUCE, "D->ncols must equal")
    if L.gf2_device_count() <= 0:
        for mname, m0 in (("P", BASE), ("D", FAR)):
            reaches_the_device_check(L, r(lo=m0 - 40, count=end(m0), hi=end(m0) + 8))          # right before, right behind
        reaches_the_device_check(L, sort(L, P, c0=0, b=b, order=BASE - 40, skeys=end(BASE)))
        reaches_the_device_check(L, sort(L, P, c0=0, b=b, order=ORDER, skeys=ORDER + 40))       # side by side
        reaches_the_device_check(L, r(count=LO - 8, lo=LO, hi=LO + 40))
        # a null array meets nothing; with no room in D lo and hi are empty
        reaches_the_device_check(L, r(lo=None, hi=None))
        reaches_the_device_check(L, sort(L, P, c0=0, b=b, order=ORDER, skeys=None))
        reaches_the_device_check(L, reduce(L, pkg, P, D=mat(pkg, 0, 200, None), c0=0, b=b, lo=BASE, hi=BASE))
        reaches_the_device_check(L, sort(L, mat(pkg, 0, 200, None), c0=0, b=b, order=ORDER, skeys=ORDER))   # no row: empty arrays


def test_d_may_share_no_word_with_p(pkg, L):
    P = mat(pkg, 10, 200, BASE, 6)
    r = lambda D, **kw: reduce(L, pkg, P, D=D, c0=0, b=4, **kw)  # noqa: E731
    refused(L, r(mat(pkg, 10, 200, BASE, 6)), REDUCE, "overlap", "D", "P")                   # in place
    refused(L, r(mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)), REDUCE, "overlap", "D", "P")        # some of P's rows
    refused(L, r(mat(pkg, 10, 200, BASE + 8 * 3, 6)), REDUCE, "overlap", "D", "P")           # shifted by three words: shares one
    refused(L, r(mat(pkg, 10, 200, BASE - 8 * 6 * 9, 6)), REDUCE, "overlap", "D", "P")       # its last row is P's first
    refused(L, r(mat(pkg, 10, 200, BASE + 8, 8)), REDUCE, "overlap", "D", "P")               # another ld: address ranges
    refused(L, r(mat(pkg, 10, 200, BASE, 6), count=COUNT + 4), REDUCE, "count is not 8-byte aligned")   # bad arguments first
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, r(mat(pkg, 10, 200, BASE + 8 * 6 * 10, 6)))              # right behind
        reaches_the_device_check(L, r(mat(pkg, 10, 200, BASE - 8 * 6 * 10, 6)))              # right before
        P12 = mat(pkg, 10, 200, BASE, 12)
        reaches_the_device_check(L, reduce(L, pkg, P12, D=mat(pkg, 10, 200, BASE + 8 * 4, 12), c0=0, b=4))
        refused(L, reduce(L, pkg, P12, D=mat(pkg, 10, 200, BASE + 8 * 3, 12), c0=0, b=4), REDUCE, "overlap", "D", "P")


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, nrows, ncols, b):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    return L.gf2_lf2_plan(nrows, ncols, b, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    nrows = 100003
    lanes_by_width = []
    for words in (1, 2, 3, 4, 5, 64, 65):
        ncols = 64 * words - 3
        seen = set()
        for b in range(31):
            passes, o = plan(L, nrows, ncols, b)
            bits, threads, lds, T, R, lanes, sort_bytes, reduce_bytes = o
            assert 1 <= bits <= 8 and passes == -(-b // bits) == -(-b // 8), (b, o)       # ceil(b / 8), none for b == 0
            assert threads in (64, 128, 256, 512, 1024) and 0 < lds <= 160 * 1024, (b, o)
            assert T >= threads and T % threads == 0 and R >= threads and R % threads == 0, (b, o)
            assert lanes in (1, 2, 8, 64), (b, o)
            tiles = -(-nrows // T)
            assert sort_bytes >= 16 * nrows + 4 * (1 << bits) * tiles, (b, o)    # two pair buffers and a tile's digit counts
            assert reduce_bytes >= sort_bytes + 8 * nrows + 8 * -(-nrows // R), (b, o)    # ... order, skeys, run sums
            assert device.lf2_plan(nrows, ncols, b) == (passes,) + tuple(o)
            seen.add((bits, threads, lds, T, R, lanes, sort_bytes, reduce_bytes))
        assert len(seen) == 1                                # all but the passes follow the shape alone
        lanes_by_width.append(lanes)
    assert lanes_by_width == sorted(lanes_by_width) and lanes_by_width[0] == 1     # wider rows never get fewer lanes
    assert lanes_by_width[2] == lanes_by_width[3] and lanes_by_width[4] == lanes_by_width[5] < lanes_by_width[6]
    # the counts of a pass shrink with the tile: at 2^26 rows a two-level scan of chunks of at least 1024 covers them
    passes, o = plan(L, 1 << 26, 256, 24)
    assert passes == 3 and 256 * ((1 << 26) // o[3]) <= 1024 * 1024 * 16
    assert plan(L, 0, 256, 8)[0] == 1 and plan(L, 1, 256, 8)[1][6] >= 16
    for bad in ((-1, 256, 8), (10, -1, 8), (10, 256, -1), (10, 256, 31)):
        assert plan(L, *bad) == (-1, [-7] * 8)
        assert device.lf2_plan(*bad) is None
    assert L.gf2_lf2_plan(10, 256, 20, None) == 3 and L.gf2_lf2_plan(10, 256, 31, None) == -1
