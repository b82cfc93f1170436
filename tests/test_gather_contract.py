"""CPU tests of the contract of include/m4ri_hip_gather.h (gf2_gather_rows_dev, gf2_gather_cols_dev, gf2_gather_cols_plan): every
argument is checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around
addresses that are never dereferenced (the BASE / FAR technique of tests/test_dev_contract.py).

Two rules of older tests are restated here for the companion header, because their own lists are closed:
  * tests/test_host_abi.py::test_header_symbols_are_exported -- every gf2_* the header declares is exported, and the binding's table for
    this header (_lib.GATHER_SYMBOLS) names exactly those;
  * tests/test_dev_contract.py::test_every_entry_with_two_matrices_has_a_stated_rule -- every function of the header that takes two
    gf2_dmat states its aliasing rule at its declaration (RULE_WORDS below are the words looked for)."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_gather.h")

BASE = 1 << 20   # an address that is never dereferenced
FAR = 1 << 28    # a second buffer, far from the first
IDX = 1 << 30    # where the index array would be
BAD = (1 << 30) + (1 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

ROWS, COLS = "gf2_gather_rows_dev", "gf2_gather_cols_dev"
# the words that state the aliasing rule at a declaration of the header
RULE_WORDS = ("Aliasing:", "may share no word with S", '"overlap"', "idx and bad may not meet D's address range")


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


def call(L, name, D, S, idx=IDX, bad=None, accumulate=0):
    if name == ROWS:
        return L.gf2_gather_rows_dev(ref(D), ref(S), idx, accumulate, bad, None)
    return L.gf2_gather_cols_dev(ref(D), ref(S), idx, bad, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


def shapes(name):
    """(D shape, S shape) of a good call: rows 7 <- 10 of 200 columns; columns 10 x 70 <- 10 x 200"""
    return ((7, 200), (10, 200)) if name == ROWS else ((10, 70), (10, 200))


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_gather.h"\nint main(void){ gf2_dmat d; (void)d; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {ROWS, COLS, "gf2_gather_cols_plan"}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.GATHER_SYMBOLS)
    assert not declared & set(pkg._lib.DECLARED_SYMBOLS)   # that list stays the one of m4ri_hip.h


def test_every_entry_with_two_matrices_states_its_aliasing_rule():
    text = open(HEADER).read()
    two = [n for n, args in declarations().items() if len(re.findall(r"\bgf2_dmat\b", args)) >= 2]
    assert sorted(two) == [COLS, ROWS]
    for name in two:
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]   # the comment that ends right above the declaration
        assert comment.rstrip().endswith("*/"), name
        for w in RULE_WORDS:
            assert w in comment, (name, w)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [ROWS, COLS])
def test_argument_errors(pkg, L, name):
    (dr, dc), (sr, sc) = shapes(name)
    D, S = mat(pkg, dr, dc, FAR), mat(pkg, sr, sc, BASE)
    refused(L, call(L, name, None, S), name, "D is null")
    refused(L, call(L, name, D, None), name, "S is null")
    refused(L, call(L, name, mat(pkg, dr, dc, None), S), name, "D.data is null")
    refused(L, call(L, name, D, mat(pkg, sr, sc, None)), name, "S.data is null")
    refused(L, call(L, name, D, S, idx=None), name, "idx is null")
    refused(L, call(L, name, mat(pkg, -1, dc, FAR), S), name, "negative")
    refused(L, call(L, name, mat(pkg, dr, -dc, FAR), S), name, "negative")
    refused(L, call(L, name, D, mat(pkg, -sr, sc)), name, "negative")
    refused(L, call(L, name, D, mat(pkg, sr, -1)), name, "negative")
    refused(L, call(L, name, mat(pkg, dr, dc, FAR, ld=width(dc) - 1), S), name, "D.ld is smaller")
    refused(L, call(L, name, D, mat(pkg, sr, sc, ld=width(sc) - 1)), name, "S.ld is smaller")
    refused(L, call(L, name, mat(pkg, dr, dc, FAR + 4), S), name, "D.data is not 8-byte aligned")
    refused(L, call(L, name, D, mat(pkg, sr, sc, BASE + 1)), name, "S.data is not 8-byte aligned")
    if name == ROWS:
        refused(L, call(L, name, mat(pkg, dr, dc + 1, FAR), S), name, "shape mismatch")
        refused(L, call(L, name, mat(pkg, dr, dc - 1, FAR), S, accumulate=1), name, "shape mismatch")
    else:
        refused(L, call(L, name, mat(pkg, dr + 1, dc, FAR), S), name, "shape mismatch")
        refused(L, call(L, name, mat(pkg, dr - 1, dc, FAR), S), name, "shape mismatch")
    # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, call(L, name, mat(pkg, dr, dc, FAR + 8, ld=width(dc) + 1), mat(pkg, sr, sc, BASE + 8, ld=width(sc) + 3)))


@pytest.mark.parametrize("name", [ROWS, COLS])
def test_an_empty_destination_is_no_error_and_needs_no_device(pkg, L, name):
    if name == ROWS:
        cases = [((0, 200), (10, 200)), ((7, 0), (10, 0)), ((0, 0), (0, 0)), ((0, 200), (0, 200))]
    else:
        cases = [((10, 0), (10, 200)), ((0, 70), (0, 200)), ((0, 0), (0, 0)), ((10, 0), (10, 0))]
    for (dr, dc), (sr, sc) in cases:
        for idx in (IDX, None):
            assert call(L, name, mat(pkg, dr, dc, None), mat(pkg, sr, sc, BASE if sr and sc else None), idx=idx) == 0
    # empty and on top of S: nothing is written, nothing is refused
    (dr, dc), (sr, sc) = cases[0]
    assert call(L, name, mat(pkg, dr, dc, BASE), mat(pkg, sr, sc, BASE)) == 0
    # an empty S under a non-empty D is a zero D: not an argument error (it needs the device)
    if L.gf2_device_count() <= 0:
        empty = ((7, 200), (0, 200)) if name == ROWS else ((10, 70), (10, 0))
        reaches_the_device_check(L, call(L, name, mat(pkg, *empty[0], FAR), mat(pkg, *empty[1], None)))


# ---- aliasing -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [ROWS, COLS])
def test_a_destination_on_the_source_is_refused(pkg, L, name):
    (dr, dc), (sr, sc) = shapes(name)
    sld = 4
    placements = [("the same base", BASE, sld), ("one row in", BASE + 8 * sld, sld), ("one word in", BASE + 8, sld),
                  ("the same base, another ld", BASE, sld + 2), ("its last row is the other's first", BASE - 8 * sld * (dr - 1), sld),
                  ("its last word is the other's first", BASE - 8 * (width(dc) - 1), sld)]
    for what, data, ld in placements:
        for accumulate in ((0, 1) if name == ROWS else (0,)):
            rc = call(L, name, mat(pkg, dr, dc, data, ld), mat(pkg, sr, sc, BASE, sld), accumulate=accumulate)
            refused(L, rc, name, "overlap", "D and S")


@pytest.mark.parametrize("name", [ROWS, COLS])
def test_index_and_flag_inside_the_destination_are_refused(pkg, L, name):
    (dr, dc), (sr, sc) = shapes(name)
    D, S = mat(pkg, dr, dc, FAR, 4), mat(pkg, sr, sc, BASE, 4)
    count = dr if name == ROWS else dc
    last = FAR + 8 * ((dr - 1) * 4 + width(dc))        # the first byte behind D's last word
    for idx in (FAR, FAR + 8 * 4 + 4, last - 4, FAR - 4 * count + 4):
        refused(L, call(L, name, D, S, idx=idx), name, "overlap", "idx")
    for bad in (FAR, FAR + 12, last - 4):
        refused(L, call(L, name, D, S, bad=bad), name, "overlap", "bad")
    if L.gf2_device_count() <= 0:
        # right before and right behind D; idx inside S is allowed (S is only read)
        reaches_the_device_check(L, call(L, name, D, S, idx=FAR - 4 * count, bad=last))
        reaches_the_device_check(L, call(L, name, D, S, idx=last, bad=FAR - 4))
        reaches_the_device_check(L, call(L, name, D, S, idx=BASE, bad=BAD))


@pytest.mark.parametrize("name", [ROWS, COLS])
def test_two_column_ranges_of_one_parent_pass_the_overlap_check(pkg, L, name):
    if L.gf2_device_count() > 0:
        return  # with a device the call would run: tests/test_gpu_gather.py runs it
    (dr, dc), (sr, sc) = shapes(name)
    rows = max(dr, sr)
    # a parent of 8 words per row: S in words 0 .. 3, D in words 4 .. 7 (rows: D's 7 rows beside S's first 7)
    S, D = mat(pkg, sr if name == ROWS else rows, sc, BASE, 8), mat(pkg, dr if name == ROWS else rows, dc, BASE + 32, 8)
    reaches_the_device_check(L, call(L, name, D, S, idx=IDX, bad=BAD))
    # ... and one word to the left they meet
    refused(L, call(L, name, mat(pkg, D.nrows, dc, BASE + 24, 8), S), name, "overlap")


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, nrows, s_ncols, d_ncols):
    out = (ctypes.c_longlong * 4)(-7, -7, -7, -7)
    return L.gf2_gather_cols_plan(nrows, s_ncols, d_ncols, out), list(out)


def first_composed(L, nrows=70):
    lo, hi = 1, 1 << 24   # fused at lo, composed at hi
    assert plan(L, nrows, lo, lo)[0] == 0 and plan(L, nrows, hi, 64)[0] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(L, nrows, mid, 64)[0] == 0 else (lo, mid)
    return hi


def test_plan(pkg, L):
    LDS_PER_WORKGROUP = 163840
    for nrows, s, d in ((1, 1, 1), (64, 64, 64), (257, 4133, 4096), (65536, 8192, 8192), (70, 0, 5)):
        path, (threads, lds, rows, scratch) = plan(L, nrows, s, d)
        assert path == 0 and threads in (64, 128, 256, 512, 1024) and rows > 0 and rows % 64 == 0 and scratch == 0, (nrows, s, d)
        assert 8 * s <= lds <= LDS_PER_WORKGROUP, (s, lds)   # 8 bytes per source column at the least
    edge = first_composed(L)
    assert edge > 4133
    for s in (edge, edge + 1, 1 << 20):
        path, (threads, lds, rows, scratch) = plan(L, 70, s, 100)
        assert path == 1 and lds == 0 and scratch >= 8 * (s + 100) * width(70), (s, scratch)
    path, (threads, lds, rows, scratch) = plan(L, 70, edge - 1, 100)
    assert path == 0 and lds <= LDS_PER_WORKGROUP
    # monotone: no fused shape above the edge, no composed one below it (the edge does not depend on the other two dimensions)
    for s in range(1, edge + 200, 61):
        for nrows, d in ((1, 1), (100000, 3), (64, 100000)):
            assert plan(L, nrows, s, d)[0] == (0 if s < edge else 1), (nrows, s, d)
    for shape in ((-1, 5, 5), (5, -1, 5), (5, 5, -1)):
        assert plan(L, *shape)[0] == -1
    assert L.gf2_gather_cols_plan(70, 100, 100, None) == 0   # out may be NULL
    from m4ri_rust_amd import device
    assert device.gather_cols_plan(70, 100, 100)[0] == 0 and device.gather_cols_plan(70, edge, 100)[0] == 1
    assert device.gather_cols_plan(-1, 100, 100) is None
