"""CPU tests of the contract of include/m4ri_hip_weight.h (gf2_row_weights_dev, gf2_col_weights_dev, gf2_count_ones_dev,
gf2_select_weights_dev, gf2_weights_plan): every argument is checked before a device is required and before the first HIP call, so
this runs without one, on DMatStructs around addresses that are never dereferenced (the BASE / FAR technique of
tests/test_gather_contract.py).

The rule of tests/test_host_abi.py::test_header_symbols_are_exported is restated here for this companion header, because its own
list is closed: every gf2_* the header declares is exported, and the binding's table for this header (_lib.WEIGHT_SYMBOLS) names
exactly those."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_weight.h")

BASE = 1 << 20   # an address that is never dereferenced
FAR = 1 << 28    # a second buffer, far from the first
IDX = 1 << 30    # where the index array would be
CNT = (1 << 30) + (1 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

ROWS, COLS, TOTAL, SELECT, PLAN = ("gf2_row_weights_dev", "gf2_col_weights_dev", "gf2_count_ones_dev", "gf2_select_weights_dev",
                                   "gf2_weights_plan")
MATRIX_ENTRIES = (ROWS, COLS, TOTAL)
OUT_NAME = {ROWS: "weights", COLS: "weights", TOTAL: "total"}
OUT_ALIGN = {ROWS: 4, COLS: 4, TOTAL: 8}


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


def call(L, name, A, out=FAR):
    return getattr(L, name)(ref(A), out, None)


def select(L, weights=BASE, n=100, lo=0, hi=5, idx=IDX, cap=100, count=CNT):
    return L.gf2_select_weights_dev(weights, n, lo, hi, idx, cap, count, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


def out_len(name, A):
    return {ROWS: A.nrows, COLS: A.ncols, TOTAL: 1}[name]


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_weight.h"\nint main(void){ gf2_dmat d; (void)d; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {ROWS, COLS, TOTAL, SELECT, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.WEIGHT_SYMBOLS)
    assert not declared & set(pkg._lib.DECLARED_SYMBOLS)   # that list stays the one of m4ri_hip.h
    assert not declared & set(pkg._lib.GATHER_SYMBOLS)


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("OVERWRITTEN", "from min(*count, cap) on are not touched", "no host synchronisation and no hipMalloc",
                  "has been written by the same call", "never read", "16-byte loads are used only where", "without a device",
                  "count-only call", '"overlap"', "64-bit offsets"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MATRIX_ENTRIES)
def test_argument_errors(pkg, L, name):
    A = mat(pkg, 10, 200)
    o = OUT_NAME[name]
    refused(L, call(L, name, None), name, "A is null")
    refused(L, call(L, name, mat(pkg, 10, 200, None)), name, "A.data is null")
    refused(L, call(L, name, A, None), name, o + " is null")
    refused(L, call(L, name, mat(pkg, -1, 200)), name, "negative")
    refused(L, call(L, name, mat(pkg, 10, -200)), name, "negative")
    refused(L, call(L, name, mat(pkg, 10, 200, ld=width(200) - 1)), name, "A.ld is smaller")
    refused(L, call(L, name, mat(pkg, 10, 200, BASE + 4)), name, "A.data is not 8-byte aligned")
    refused(L, call(L, name, A, FAR + 2), name, "%s is not %d-byte aligned" % (o, OUT_ALIGN[name]))
    if name == TOTAL:
        refused(L, call(L, name, A, FAR + 4), name, "total is not 8-byte aligned")
    assert L.gf2_last_error().decode().startswith(name)
    if L.gf2_device_count() <= 0:
        # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
        reaches_the_device_check(L, call(L, name, mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, call(L, name, A, FAR + (4 if name != TOTAL else 8)))


@pytest.mark.parametrize("name", MATRIX_ENTRIES)
def test_an_output_inside_the_operand_is_refused(pkg, L, name):
    A = mat(pkg, 10, 200, FAR, 6)
    n = out_len(name, A)
    size = OUT_ALIGN[name]
    last = FAR + 8 * (9 * 6 + width(200))   # the first byte behind A's last word
    for out in (FAR, FAR + 8 * 6 + 8, last - size, FAR - size * n + size):
        refused(L, call(L, name, A, out), name, "overlap", OUT_NAME[name], "A")
    # the pad words between the rows belong to A's address range
    refused(L, call(L, name, A, FAR + 8 * 4), name, "overlap")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, call(L, name, A, FAR - size * n))   # right before
        reaches_the_device_check(L, call(L, name, A, last))             # right behind


def test_empty_shapes(pkg, L):
    # an output of length 0: no error, no device, nothing looked at but A itself
    for out in (FAR, None, FAR + 1):
        assert call(L, ROWS, mat(pkg, 0, 200, None), out) == 0
        assert call(L, ROWS, mat(pkg, 0, 0, None), out) == 0
        assert call(L, COLS, mat(pkg, 10, 0, None), out) == 0
        assert call(L, COLS, mat(pkg, 0, 0, None), out) == 0
    for idx in (IDX, None):
        assert select(L, weights=None, n=0, idx=idx, cap=0) == 0
        assert select(L, weights=BASE, n=0, idx=idx, cap=0) == 0
    # A itself is still checked
    refused(L, call(L, ROWS, None), ROWS, "A is null")
    refused(L, call(L, COLS, mat(pkg, -1, 0, None)), COLS, "negative")
    if L.gf2_device_count() <= 0:
        # zeros are results: an empty A under a non-empty output needs the device (data may be null: nothing is read)
        reaches_the_device_check(L, call(L, ROWS, mat(pkg, 10, 0, None)))
        reaches_the_device_check(L, call(L, COLS, mat(pkg, 0, 200, None)))
        for shape in ((0, 0), (10, 0), (0, 200)):
            reaches_the_device_check(L, call(L, TOTAL, mat(pkg, *shape, None)))
        reaches_the_device_check(L, select(L, weights=None, n=0, cap=5))   # *count = 0 is written
        reaches_the_device_check(L, select(L, lo=5, hi=4))                 # selects nothing: still writes *count
        reaches_the_device_check(L, select(L, idx=None, cap=0))            # a count-only call
    # ... and their outputs are checked like any other
    refused(L, call(L, ROWS, mat(pkg, 10, 0, None), None), ROWS, "weights is null")
    refused(L, call(L, TOTAL, mat(pkg, 0, 0, None), None), TOTAL, "total is null")


def test_select_argument_errors(pkg, L):
    refused(L, select(L, n=-1), SELECT, "n is negative")
    refused(L, select(L, cap=-1), SELECT, "cap is negative")
    refused(L, select(L, weights=None), SELECT, "weights is null")
    refused(L, select(L, count=None), SELECT, "count is null")
    refused(L, select(L, n=0, cap=0, count=None), SELECT, "count is null")
    refused(L, select(L, idx=None), SELECT, "idx is null")
    refused(L, select(L, weights=BASE + 2), SELECT, "weights is not 4-byte aligned")
    refused(L, select(L, idx=IDX + 1), SELECT, "idx is not 4-byte aligned")
    refused(L, select(L, count=CNT + 2), SELECT, "count is not 4-byte aligned")
    assert L.gf2_last_error().decode().startswith(SELECT)
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, select(L))
        reaches_the_device_check(L, select(L, weights=BASE + 4, idx=IDX + 4, count=CNT + 4))


def test_select_aliasing(pkg, L):
    n, cap = 100, 40
    for idx in (BASE, BASE + 4 * (n - 1), BASE - 4 * (cap - 1)):
        refused(L, select(L, n=n, idx=idx, cap=cap), SELECT, "overlap", "idx", "weights")
    for count in (BASE, BASE + 4 * (n - 1)):
        refused(L, select(L, n=n, cap=cap, count=count), SELECT, "overlap", "count", "weights")
    for count in (IDX, IDX + 4 * (cap - 1)):
        refused(L, select(L, n=n, cap=cap, count=count), SELECT, "overlap", "count", "idx")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, select(L, n=n, idx=BASE + 4 * n, cap=cap, count=BASE - 4))      # right behind, right before
        reaches_the_device_check(L, select(L, n=n, idx=BASE - 4 * cap, cap=cap, count=BASE + 4 * (n + cap)))
        reaches_the_device_check(L, select(L, n=n, idx=IDX, cap=cap, count=IDX + 4 * cap))         # count right behind idx's cap ints
        reaches_the_device_check(L, select(L, n=n, idx=None, cap=0, count=IDX))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, what, nrows, ncols):
    out = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    return L.gf2_weights_plan(what, nrows, ncols, out), list(out)


def row_threshold(L):
    """the first ncols of the second row variant"""
    lo, hi = 1, 1 << 24
    v0, v1 = plan(L, 0, 100, lo)[0], plan(L, 0, 100, hi)[0]
    assert v0 >= 0 and v1 >= 0 and v0 != v1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(L, 0, 100, mid)[0] == v0 else (lo, mid)
    return hi


def test_plan(pkg, L):
    for what in (0, 1, 2):
        for shape in ((-1, 5), (5, -1), (-1, -1)):
            assert plan(L, what, *shape)[0] == -1
        for shape in ((0, 0), (1, 1), (5, 0), (0, 5), (65536, 256), (1 << 20, 256), (65536, 65536), (3, 70001), ((1 << 31) - 1, (1 << 31) - 1)):
            v, (threads, rows, flush, scratch) = plan(L, what, *shape)
            assert v >= 0 and threads in (64, 128, 256, 512, 1024) and 1 <= rows <= threads and scratch >= 0, (what, shape)
            assert (flush > 0) == (what == 1), (what, shape, flush)
            if what != 1:
                assert scratch == 0
    for what in (-1, 3, 100):
        assert plan(L, what, 5, 5)[0] == -1
    assert L.gf2_weights_plan(0, 5, 5, None) == 0   # out may be NULL
    # rows: the variant changes exactly once as the width grows, whatever the row count
    T = row_threshold(L)
    assert 64 < T <= 4097
    for nrows in (1, 100, 1 << 20):
        seen = [plan(L, 0, nrows, c)[0] for c in list(range(1, 2 * T + 200)) + [4097, 70001, 1 << 24]]
        changes = sum(a != b for a, b in zip(seen, seen[1:]))
        assert changes == 1 and seen[T - 2] != seen[T - 1], (nrows, changes)
    # columns: the flush period is a constant that the six counter planes can hold; one band needs no scratch, more bands need a row
    # of ncols ints each
    v, (threads, R, F, scratch) = plan(L, 1, 3, 70001)
    assert v == 0 and scratch == 0 and 0 < F < 64
    v, (threads, R, F2, scratch) = plan(L, 1, 1 << 20, 256)
    assert v == 1 and F2 == F and scratch % (4 * 256) == 0 and scratch // (4 * 256) >= 256   # the grid fills 256 compute units
    v, (threads, R, _, scratch) = plan(L, 1, 65536, 65536)
    assert v == 1 and 0 < scratch <= 65536 * 65536 // 8 // 16   # the partial sums stay a small part of the operand
    from m4ri_rust_amd import device
    assert device.weights_plan("rows", 100, T - 1)[0] != device.weights_plan("rows", 100, T)[0]
    assert device.weights_plan("cols", 3, 70001)[:1] == (0,) and device.weights_plan("total", 5, 5) is not None
    assert device.weights_plan(0, -1, 5) is None and device.weights_plan("rows", 5, -1) is None
