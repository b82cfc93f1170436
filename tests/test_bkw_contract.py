"""CPU tests of the contract of include/m4ri_hip_bkw.h (gf2_class_first_dev, gf2_lf1_reduce_dev, gf2_lf1_plan): every argument is
checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around addresses that are
never dereferenced (the BASE / FAR technique of tests/test_wht_contract.py).

The rule of tests/test_host_abi.py::test_header_symbols_are_exported is restated here for this companion header, because its own
list is closed: every gf2_* the header declares is exported, and the binding's table for this header (_lib.BKW_SYMBOLS) names exactly
those."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_bkw.h")

BASE = 1 << 20     # P: an address that is never dereferenced
FAR = 1 << 28      # D
COUNT = 1 << 29
SRC = (1 << 29) + (1 << 20)
FIRST = 1 << 30    # the table of class firsts, above the rest: 4 GiB at b = 30
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

CLASS, REDUCE, PLAN = "gf2_class_first_dev", "gf2_lf1_reduce_dev", "gf2_lf1_plan"
ENTRIES = (CLASS, REDUCE)
KEEP_ZERO = 1


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


def first_of(L, P, c0=37, b=20, first=FIRST):
    return L.gf2_class_first_dev(ref(P), c0, b, first, None)


def reduce(L, pkg, P, D=DEFAULT, c0=37, b=20, flags=0, first=FIRST, count=COUNT, src=SRC):
    if D is DEFAULT:
        D = mat(pkg, 10, P.ncols if P is not None else 200, FAR)
    return L.gf2_lf1_reduce_dev(ref(D), ref(P), c0, b, flags, first, count, src, None)


def call(L, pkg, name, P, **kw):
    return first_of(L, P, **kw) if name == CLASS else reduce(L, pkg, P, **kw)


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
    src.write_text('#include "m4ri_hip_bkw.h"\nint main(void){ gf2_dmat d; long long o[5]; (void)d; '
                   'return gf2_lf1_plan(1, 1, 31, o) != -1 || GF2_LF1_KEEP_ZERO != 1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {CLASS, REDUCE, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.BKW_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS):   # stay what they were
        assert not declared & set(table)
    assert pkg._lib.LF1_KEEP_ZERO == KEEP_ZERO


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("OVERWRITTEN", "no host synchronisation and no hipMalloc", "has been written by the same call", "never read",
                  "at most two words", "64-bit offsets", "Nothing of P is written", "do not depend on launch order", "LOWEST index",
                  "Two runs give the same bits", "keep their order", "count-only call", "may exceed D->nrows", "are not touched",
                  "by the rule of gf2_submatrix_dev", "b == 0: every row has key 0", "nrows == 0: first is all -1", "checked last",
                  '"overlap"', "before a device is required and before the first HIP call", "no in-place round",
                  "16-byte accesses are used only where", "without a device", "work space AND output"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ENTRIES)
def test_argument_errors(pkg, L, name):
    P = mat(pkg, 10, 200)
    c = lambda P, **kw: call(L, pkg, name, P, **kw)  # noqa: E731
    refused(L, c(None), name, "P is null")
    refused(L, c(mat(pkg, 10, 200, None)), name, "P.data is null")
    refused(L, c(P, first=None), name, "first is null")
    refused(L, c(mat(pkg, -1, 200)), name, "negative")
    refused(L, c(mat(pkg, 10, -200)), name, "negative")
    refused(L, c(mat(pkg, 10, 200, ld=width(200) - 1)), name, "P.ld is smaller")
    refused(L, c(mat(pkg, 10, 200, BASE + 4)), name, "P.data is not 8-byte aligned")
    refused(L, c(P, first=FIRST + 2), name, "first is not 4-byte aligned")
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
        reaches_the_device_check(L, c(P, first=FIRST + 4))
        reaches_the_device_check(L, c(P, c0=180, b=20))     # up to the last column
        reaches_the_device_check(L, c(P, c0=50, b=30))      # over a word boundary
        reaches_the_device_check(L, c(P, c0=200, b=0))      # no window bit at all
        reaches_the_device_check(L, c(P, c0=0, b=0))
        reaches_the_device_check(L, c(mat(pkg, 0, 200, None)))   # no row: first is all -1, which still needs the device
        reaches_the_device_check(L, c(mat(pkg, 7, 0, None), c0=0, b=0))


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
    refused(L, r(count=COUNT + 1), REDUCE, "count is not 4-byte aligned")
    refused(L, r(src=SRC + 2), REDUCE, "src is not 4-byte aligned")
    for flags in (2, 3, -1, 1 << 8):
        refused(L, r(flags=flags), REDUCE, "flags", "GF2_LF1_KEEP_ZERO")
    refused(L, r(D=mat(pkg, 10, 199, FAR)), REDUCE, "D->ncols must equal P->ncols")
    refused(L, r(D=mat(pkg, 10, 256, FAR)), REDUCE, "D->ncols must equal P->ncols")
    assert L.gf2_last_error().decode().startswith(REDUCE)
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, r())
        reaches_the_device_check(L, r(flags=KEEP_ZERO))
        reaches_the_device_check(L, r(src=None))
        reaches_the_device_check(L, r(D=mat(pkg, 0, 200, None)))                    # the count-only form
        reaches_the_device_check(L, r(D=mat(pkg, 0, 200, None), src=None))
        reaches_the_device_check(L, r(D=mat(pkg, 0, 200, None), src=None, flags=KEEP_ZERO))
        reaches_the_device_check(L, r(D=mat(pkg, 1000, 200, FAR)))                  # more room than rows
        reaches_the_device_check(L, r(D=mat(pkg, 10, 200, FAR + 8, ld=width(200) + 1)))   # odd ld at an odd word, D ...
        reaches_the_device_check(L, r(P=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))  # ... and P
        reaches_the_device_check(L, r(P=mat(pkg, 0, 200, None), D=mat(pkg, 0, 200, None)))


def test_an_array_inside_an_operand_is_refused(pkg, L):
    P = mat(pkg, 10, 200, BASE, 6)
    D = mat(pkg, 10, 200, FAR, 6)
    b = 4
    nbytes = 4 << b
    end = lambda at: at + 8 * (9 * 6 + width(200))   # noqa: E731  the first byte behind the last word of a 10 x 200, ld 6
    # the class firsts alone
    for at in (BASE, BASE + 8 * 6 + 8, end(BASE) - 4, BASE - nbytes + 4, BASE + 8 * 4):   # the pad words belong to the range
        refused(L, first_of(L, P, c0=0, b=b, first=at), CLASS, "overlap", "first", "P")
    refused(L, first_of(L, P, c0=0, b=31, first=BASE), CLASS, "b = 31")            # bad arguments before the overlap
    refused(L, first_of(L, P, c0=190, b=20, first=BASE), CLASS, "outside P")
    # the reduction: every array against both matrices
    r = lambda **kw: reduce(L, pkg, P, D=D, c0=0, b=b, **kw)  # noqa: E731
    for name, size in (("first", nbytes), ("count", 4), ("src", 40)):
        for mname, m0 in (("P", BASE), ("D", FAR)):
            for at in (m0, m0 + 8 * 6 + 8, end(m0) - 4, m0 - size + 4, m0 + 8 * 4):
                refused(L, r(**{name: at}), REDUCE, "overlap", name, mname)
    # ... and against each other
    refused(L, r(first=FIRST, count=FIRST), REDUCE, "overlap", "first", "count")
    refused(L, r(first=FIRST, count=FIRST + nbytes - 4), REDUCE, "overlap", "first", "count")
    refused(L, r(first=FIRST, src=FIRST + nbytes - 4), REDUCE, "overlap", "first", "src")
    refused(L, r(first=FIRST, src=FIRST - 36), REDUCE, "overlap", "first", "src")
    refused(L, r(count=SRC, src=SRC), REDUCE, "overlap", "count", "src")
    refused(L, r(count=SRC + 36, src=SRC), REDUCE, "overlap", "count", "src")
    # bad arguments are reported before the overlap
    refused(L, reduce(L, pkg, P, D=D, c0=0, b=31, first=BASE), REDUCE, "b = 31")
    refused(L, r(first=BASE, flags=4), REDUCE, "flags")
    refused(L, r(first=BASE, count=None), REDUCE, "count is null")
    refused(L, reduce(L, pkg, P, D=mat(pkg, 10, 201, BASE, 6), c0=0, b=b), REDUCE, "D->ncols must equal")
    if L.gf2_device_count() <= 0:
        for mname, m0 in (("P", BASE), ("D", FAR)):
            reaches_the_device_check(L, r(first=m0 - nbytes, count=end(m0)))          # right before, right behind
            reaches_the_device_check(L, r(src=m0 - 40, first=end(m0), count=end(m0) + nbytes))
        reaches_the_device_check(L, first_of(L, P, c0=0, b=b, first=BASE - nbytes))
        reaches_the_device_check(L, first_of(L, P, c0=0, b=b, first=end(BASE)))
        reaches_the_device_check(L, r(first=FIRST, count=FIRST + nbytes, src=FIRST + nbytes + 4))   # side by side
        reaches_the_device_check(L, r(first=FIRST, count=FIRST - 4, src=FIRST - 44))
        # a null src meets nothing; with no room in D the src array is empty
        reaches_the_device_check(L, r(src=None))
        reaches_the_device_check(L, reduce(L, pkg, P, D=mat(pkg, 0, 200, None), c0=0, b=b, src=BASE))


def test_d_may_share_no_word_with_p(pkg, L):
    P = mat(pkg, 10, 200, BASE, 6)
    r = lambda D, **kw: reduce(L, pkg, P, D=D, c0=0, b=4, **kw)  # noqa: E731
    refused(L, r(mat(pkg, 10, 200, BASE, 6)), REDUCE, "overlap", "D", "P")                   # in place
    refused(L, r(mat(pkg, 5, 200, BASE + 8 * 6 * 3, 6)), REDUCE, "overlap", "D", "P")        # some of P's rows
    refused(L, r(mat(pkg, 10, 200, BASE + 8 * 3, 6)), REDUCE, "overlap", "D", "P")           # shifted by three words: shares one
    refused(L, r(mat(pkg, 10, 200, BASE - 8 * 6 * 9, 6)), REDUCE, "overlap", "D", "P")       # its last row is P's first
    refused(L, r(mat(pkg, 10, 200, BASE + 8, 8)), REDUCE, "overlap", "D", "P")               # another ld: address ranges
    refused(L, r(mat(pkg, 10, 200, BASE, 6), flags=2), REDUCE, "flags")                      # bad arguments first
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, r(mat(pkg, 10, 200, BASE + 8 * 6 * 10, 6)))              # right behind
        reaches_the_device_check(L, r(mat(pkg, 10, 200, BASE - 8 * 6 * 10, 6)))              # right before
        # the same stride, side by side in one parent: D in the pad words of P's rows shares no word
        P12 = mat(pkg, 10, 200, BASE, 12)
        reaches_the_device_check(L, reduce(L, pkg, P12, D=mat(pkg, 10, 200, BASE + 8 * 4, 12), c0=0, b=4))
        refused(L, reduce(L, pkg, P12, D=mat(pkg, 10, 200, BASE + 8 * 3, 12), c0=0, b=4), REDUCE, "overlap", "D", "P")


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, nrows, ncols, b):
    out = (ctypes.c_longlong * 5)(*([-7] * 5))
    return L.gf2_lf1_plan(nrows, ncols, b, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    nrows = 100003
    lanes_by_width = []
    for words in (1, 2, 3, 4, 5, 64, 65):
        ncols = 64 * words - 3
        variants, lanes = [], set()
        for b in range(31):
            v, o = plan(L, nrows, ncols, b)
            threads, lds, rows, ln, scratch = o
            assert v in (0, 1) and threads in (64, 128, 256, 512, 1024), (b, o)
            assert lds == ((4 << b) if v == 0 else 0) and lds <= 160 * 1024, (b, o)
            assert rows >= 64 and rows % 64 == 0 and ln in (1, 2, 8, 64), (b, o)
            blocks = (nrows + rows - 1) // rows
            assert scratch >= 4 * blocks, (b, o)             # an int per row block at the least
            assert device.lf1_plan(nrows, ncols, b) == (v, threads, lds, rows, ln, scratch)
            variants.append(v)
            lanes.add(ln)
        assert sum(a != c for a, c in zip(variants, variants[1:])) == 1 and variants[0] == 0 and variants[-1] == 1, variants
        assert len(lanes) == 1                               # the lanes follow the width alone
        lanes_by_width.append(lanes.pop())
    assert lanes_by_width == sorted(lanes_by_width) and lanes_by_width[0] == 1     # wider rows never get fewer lanes
    assert lanes_by_width[2] == lanes_by_width[3] and lanes_by_width[4] == lanes_by_width[5] < lanes_by_width[6]   # 3..4 words, 5..64, above
    # no row: no block, no scratch; one row: one block
    assert plan(L, 0, 256, 8)[1][4] == 0 and plan(L, 1, 256, 8)[1][4] >= 4
    for bad in ((-1, 256, 8), (10, -1, 8), (10, 256, -1), (10, 256, 31)):
        assert plan(L, *bad) == (-1, [-7] * 5)
        assert device.lf1_plan(*bad) is None
    assert L.gf2_lf1_plan(10, 256, 20, None) == plan(L, 10, 256, 20)[0] and L.gf2_lf1_plan(10, 256, 31, None) == -1
