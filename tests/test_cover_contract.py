"""CPU tests of the contract of include/m4ri_hip_cover.h (gf2_cover_code_named, gf2_cover_leaders, gf2_cover_reduce_dev, gf2_cover_plan):
every argument is checked before a device is required and before the first HIP call, so this runs without one, on DMatStructs around
addresses that are never dereferenced (the BASE / FAR technique of tests/test_bkw_contract.py).  Codes, segment indices and the array of
table pointers are host memory and real; the table pointers in it are device addresses and made up.

The rule of tests/test_host_abi.py::test_header_symbols_are_exported is restated here for this companion header, because its own
list is closed: every gf2_* the header declares is exported, and the binding's table for this header (_lib.COVER_SYMBOLS) names
exactly those."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cover_ref as cr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_cover.h")

BASE = 1 << 20     # P: an address that is never dereferenced
FAR = 1 << 28      # D
DIST = 1 << 29
TAB = 1 << 30      # table c at TAB + c * TAB_STEP
TAB_STEP = 1 << 16
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

NAMED, LEADERS, REDUCE, PLAN = "gf2_cover_code_named", "gf2_cover_leaders", "gf2_cover_reduce_dev", "gf2_cover_plan"
GOLAY, HAM3, ID1, REP13 = cr.golay23(), cr.hamming(3), cr.identity(1), cr.repetition(13)
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


def code_array(pkg, codes):
    arr = (pkg._lib.CoverCodeStruct * max(len(codes), 1))()
    for i, c in enumerate(codes):
        arr[i].n, arr[i].k = c.n, c.k
        for t, row in enumerate(c.h):
            arr[i].h[t] = row
    return arr


def reduce(L, pkg, P=DEFAULT, D=DEFAULT, c0=37, codes=(GOLAY, HAM3, ID1), seg=(0, 1, 2), tables=DEFAULT, dist=DIST, ncodes=None, nseg=None,
           no_codes=False, no_seg=False, no_tables=False):
    """one gf2_cover_reduce_dev call; by default 10 x 200 at BASE, 31 window bits from column 37 on, D 10 x K at FAR"""
    K = sum(codes[c].k for c in seg if c < len(codes))
    if P is DEFAULT:
        P = mat(pkg, 10, 200)
    if D is DEFAULT:
        D = mat(pkg, P.nrows if P is not None else 10, K, FAR)
    if tables is DEFAULT:
        tables = [TAB + c * TAB_STEP for c in range(len(codes))]
    ta = (ctypes.c_void_p * max(len(tables), 1))(*tables)
    sa = (ctypes.c_ubyte * max(len(seg), 1))(*seg)
    return L.gf2_cover_reduce_dev(ref(D), ref(P), c0, None if no_codes else code_array(pkg, codes), len(codes) if ncodes is None else ncodes,
                                  None if no_seg else sa, len(seg) if nseg is None else nseg, None if no_tables else ta, dist, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert msg.startswith(REDUCE) and all(w in msg for w in words), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_cover.h"\nint main(void){ gf2_dmat d; gf2_cover_code c; long long o[8]; (void)d; '
                   '_Static_assert(sizeof(gf2_cover_code) == 56, "56 bytes");\n'
                   'return gf2_cover_code_named(GF2_COVER_GOLAY23, 0, &c) || gf2_cover_plan(1, 64, &c, 1, 0, 0, o) < 0 || '
                   'GF2_COVER_MAX_LEADERS != 16384 || GF2_COVER_MAX_SEGS != 256 || GF2_COVER_MAX_CODES != 16 || GF2_COVER_MAX_N != 32 || '
                   'GF2_COVER_MAX_R != 12 || GF2_COVER_IDENTITY != 0 || GF2_COVER_GOLAY23 != 4; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {NAMED, LEADERS, REDUCE, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.COVER_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS):
        assert not declared & set(table)                                                      # they stay what they were
    lib = pkg._lib
    assert (lib.COVER_MAX_N, lib.COVER_MAX_R, lib.COVER_MAX_CODES, lib.COVER_MAX_SEGS, lib.COVER_MAX_LEADERS) == (32, 12, 16, 256, 16384)
    assert (lib.COVER_IDENTITY, lib.COVER_DROP, lib.COVER_REPETITION, lib.COVER_HAMMING, lib.COVER_GOLAY23) == (0, 1, 2, 3, 4)


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("OVERWRITTEN", "no host synchronisation, no hipMalloc and no scratch", "kernel arguments", "never read",
                  "Only the window bits of P are read", "at most two words", "64-bit offsets", "Nothing of P is written",
                  "does not depend on launch order", "Two runs give the same bits", "by the rule of gf2_submatrix_dev",
                  "keeps its neighbouring words", "LOWEST weight", "smallest as an integer", "O(2^r n)", "h[t] >> k == 1u << t",
                  "r == 0 is the identity code", "k == 0 is the zero code", "taken as they are", "nrows == 0 nothing is launched",
                  "only dist is written", "checked last", '"overlap"', "before a device is required and before the first HIP call",
                  "no in-place call", "16-byte accesses are used only where", "without a device", "copied into LDS once per workgroup",
                  "x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1", "1, 23, 253, 1771", "h[t] = 1 | 1 << (1 + t)", "not a power of two"):
        assert words in text, words


# ---- the named codes and the leaders ----------------------------------------------------------------------------------------------------

def named(L, pkg, kind, param):
    s = pkg._lib.CoverCodeStruct()
    s.n = s.k = -7
    rc = L.gf2_cover_code_named(kind, param, ctypes.byref(s))
    return rc, s


def as_ref(s):
    r = s.n - s.k if 0 < s.k < s.n else 0
    return cr.Code(s.n, s.k, tuple(s.h[t] for t in range(r)))


NAMED_CODES = ([(0, n, cr.identity(n)) for n in range(1, 33)] + [(1, n, cr.drop(n)) for n in range(1, 33)] +
               [(2, n, cr.repetition(n)) for n in range(2, 14)] + [(3, r, cr.hamming(r)) for r in range(2, 6)] + [(4, 0, cr.golay23())])


def test_named_codes_and_their_leaders(L, pkg):
    from m4ri_rust_amd import device
    for kind, param, want in NAMED_CODES:
        rc, s = named(L, pkg, kind, param)
        assert rc == 0 and as_ref(s) == want, (kind, param)
        assert all(s.h[t] == 0 for t in range(len(want.h), 12)), (kind, param)
        r = want.n - want.k
        out = np.full((1 << min(r, 12)) + 1, 0xDEADBEEF, dtype=np.uint32)
        radius = ctypes.c_int(-7)
        assert L.gf2_cover_leaders(ctypes.byref(s), out.ctypes.data, ctypes.byref(radius)) == 0
        table, want_radius = cr.leaders(want)
        if want.k == 0:
            assert np.all(out == 0xDEADBEEF) and radius.value == 0          # nothing is written
        else:
            assert np.array_equal(out[:len(table)], table) and np.all(out[len(table):] == 0xDEADBEEF), (kind, param)
            assert radius.value == want_radius
        assert L.gf2_cover_leaders(ctypes.byref(s), out.ctypes.data, None) == 0     # radius may be NULL
    makers = [device.CoverCode.identity, device.CoverCode.drop, device.CoverCode.repetition, device.CoverCode.hamming]
    for kind, param, want in NAMED_CODES:
        code = makers[kind](param) if kind < 4 else device.CoverCode.golay23()
        table, radius = cr.leaders(want)
        assert (code.n, code.k, code.h[:len(want.h)]) == want and code.radius == radius
        assert code.leaders().dtype == np.uint32 and np.array_equal(code.leaders(), table)
        assert code == device.CoverCode.from_rows(want.n, want.k, want.h) and code.has_table == cr.has_table(want)
    for kind, bad in ((0, (0, 33, -1)), (1, (0, 33)), (2, (1, 14, 0)), (3, (1, 6, 0)), (4, (1, -1, 23)), (5, (0, 3)), (-1, (3,))):
        for param in bad:
            rc, s = named(L, pkg, kind, param)
            assert rc == -1 and (s.n, s.k) == (-7, -7), (kind, param)
    assert L.gf2_cover_code_named(0, 5, None) == -1
    with pytest.raises(ValueError):
        device.CoverCode.hamming(6)


def random_systematic(n, k, seed):
    rng = np.random.default_rng(seed)
    return cr.Code(n, k, tuple(int(rng.integers(0, 1 << k)) | 1 << (k + t) for t in range(n - k)))


def test_leaders_of_other_codes_and_of_bad_ones(L, pkg):
    from m4ri_rust_amd import device
    for n, k, seed in ((12, 6, 5), (20, 10, 1), (32, 26, 2), (30, 18, 7), (13, 1, 3), (32, 31, 4), (24, 12, 6)):
        want = random_systematic(n, k, seed)
        code = device.CoverCode.from_rows(n, k, want.h)
        table, radius = cr.leaders(want)
        assert np.array_equal(code.leaders(), table) and code.radius == radius, (n, k)
    out = np.zeros(1 << 12, dtype=np.uint32)
    ham = cr.hamming(3)
    for bad in (cr.Code(0, 0, ()), cr.Code(33, 33, ()), cr.Code(33, 0, ()), cr.Code(5, -1, ()), cr.Code(5, 6, ()),
                cr.Code(14, 1, tuple(1 | 1 << (1 + t) for t in range(12))),          # r = 13 (the thirteenth row does not fit anyway)
                cr.Code(7, 4, (ham.h[0] | 1 << 7, ham.h[1], ham.h[2])),              # a bit at n
                cr.Code(7, 4, (ham.h[0] | 1 << 31, ham.h[1], ham.h[2])),
                cr.Code(7, 4, (ham.h[1], ham.h[0], ham.h[2])),                       # not systematic: rows swapped
                cr.Code(7, 4, (ham.h[0] | 1 << 5, ham.h[1], ham.h[2])),              # ... a second bit in the identity part
                cr.Code(7, 4, (ham.h[0], ham.h[1], ham.h[2] & 15))):                 # ... a row without its own
        arr = code_array(pkg, [bad])
        assert L.gf2_cover_leaders(arr, out.ctypes.data, None) == -1, bad
        assert L.gf2_cover_plan(10, 64, arr, 1, None, 0, None) == -1, bad
        with pytest.raises(ValueError):
            device.CoverCode.from_rows(bad.n, bad.k, bad.h)
    assert L.gf2_cover_leaders(None, out.ctypes.data, None) == -1
    # identity and drop read no h: rows that would be illegal are ignored, and n may be 32
    for n, k in ((32, 32), (32, 0), (9, 9), (9, 0)):
        arr = code_array(pkg, [cr.Code(n, k, (0xFFFFFFFF,) * 12)])
        out[:2] = 0xDEADBEEF
        assert L.gf2_cover_leaders(arr, out.ctypes.data, None) == 0
        assert list(out[:2]) == ([0, 0xDEADBEEF] if k else [0xDEADBEEF] * 2)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_argument_errors(pkg, L):
    r = lambda **kw: reduce(L, pkg, **kw)  # noqa: E731
    refused(L, r(P=None), "P is null")
    refused(L, r(D=None), "D is null")
    refused(L, r(P=mat(pkg, 10, 200, None)), "P.data is null")
    refused(L, r(D=mat(pkg, 10, 17, None)), "D.data is null")
    refused(L, r(P=mat(pkg, -1, 200)), "negative")
    refused(L, r(D=mat(pkg, 10, -17, FAR)), "negative")
    refused(L, r(P=mat(pkg, 10, 200, ld=width(200) - 1)), "P.ld is smaller")
    refused(L, r(D=mat(pkg, 10, 130, FAR, ld=2), seg=(0,) * 10 + (1, 1, 2, 2), c0=0), "D.ld is smaller")
    refused(L, r(P=mat(pkg, 10, 200, BASE + 4)), "P.data is not 8-byte aligned")
    refused(L, r(D=mat(pkg, 10, 17, FAR + 4)), "D.data is not 8-byte aligned")
    refused(L, r(dist=DIST + 2), "dist is not 4-byte aligned")
    for n in (0, 17, -1):
        refused(L, r(ncodes=n), "ncodes = %d" % n, "1 <= ncodes <= 16")
    refused(L, r(codes=(GOLAY,) * 17, seg=(16,)), "ncodes = 17")
    for n in (-1, 257, 1 << 20):
        refused(L, r(nseg=n), "nseg = %d" % n, "0 <= nseg <= 256")
    refused(L, r(no_codes=True), "codes is null")
    refused(L, r(no_seg=True), "seg_code is null")
    refused(L, r(no_tables=True), "leaders is null")
    refused(L, r(seg=(0, 1, 3)), "seg_code[2] = 3", "ncodes = 3")
    refused(L, r(seg=(255, 1, 2)), "seg_code[0] = 255")
    ham = HAM3
    for bad, why in ((cr.Code(0, 0, ()), "1 <= n <= 32"), (cr.Code(33, 0, ()), "1 <= n <= 32"), (cr.Code(5, -1, ()), "0 <= k <= n"),
                     (cr.Code(5, 6, ()), "0 <= k <= n"), (cr.Code(14, 1, tuple(1 | 1 << (1 + t) for t in range(12))), "above 12"),
                     (cr.Code(7, 4, (ham.h[0] | 1 << 7, ham.h[1], ham.h[2])), "at or above n"),
                     (cr.Code(7, 4, (ham.h[1], ham.h[0], ham.h[2])), "not systematic")):
        refused(L, r(codes=(GOLAY, bad, ID1)), "codes[1]", why)
        refused(L, r(codes=(GOLAY, ID1, bad), seg=(0, 1)), "codes[2]", why)          # also where no segment uses it
    refused(L, r(tables=[TAB, None, None]), "leaders[1] is null")
    refused(L, r(tables=[None, TAB, None]), "leaders[0] is null")
    refused(L, r(tables=[TAB + 2, TAB + TAB_STEP, None]), "leaders[0] is not 4-byte aligned")
    refused(L, r(codes=(REP13,) * 5, seg=(0,), tables=[TAB] * 5), "20480 words", "GF2_COVER_MAX_LEADERS")
    refused(L, r(codes=(REP13,) * 4 + (HAM3,), seg=(4,), tables=[TAB] * 5), "16392 words")    # also where no segment uses them
    refused(L, r(c0=-1), "window", "outside P")
    refused(L, r(c0=170), "window", "[170, 201)", "outside P")
    refused(L, r(c0=(1 << 31) - 1), "window", "outside P")
    refused(L, r(D=mat(pkg, 10, 16, FAR)), "D->ncols must equal K", "K = 17")
    refused(L, r(D=mat(pkg, 10, 31, FAR)), "D->ncols must equal K")
    refused(L, r(D=mat(pkg, 10, 17, FAR), nseg=0), "D->ncols must equal K", "K = 0")
    refused(L, r(D=mat(pkg, 9, 17, FAR)), "D->nrows must equal P->nrows")
    refused(L, r(D=mat(pkg, 11, 17, FAR)), "D->nrows must equal P->nrows")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, r())
        reaches_the_device_check(L, r(dist=None))
        reaches_the_device_check(L, r(dist=DIST + 4))
        # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
        reaches_the_device_check(L, r(P=mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, r(D=mat(pkg, 10, 17, FAR + 8, ld=3)))
        reaches_the_device_check(L, r(c0=169))                                        # a window that ends at the last column
        reaches_the_device_check(L, r(c0=0))
        reaches_the_device_check(L, r(tables=[TAB, TAB + 4, None]))                   # identity needs no table ...
        reaches_the_device_check(L, r(codes=(GOLAY, HAM3, ID1, REP13), tables=[TAB, TAB + 64, None, None]))    # ... nor a code no segment uses
        reaches_the_device_check(L, r(seg=(), D=mat(pkg, 10, 0, None)))               # nseg == 0: only dist is written
        reaches_the_device_check(L, r(seg=(), D=mat(pkg, 10, 0, None), codes=(), no_codes=True, no_seg=True, no_tables=True))
        reaches_the_device_check(L, r(codes=(cr.drop(12), ID1), seg=(0, 0), D=mat(pkg, 10, 0, None), no_tables=True))      # K == 0
        reaches_the_device_check(L, r(P=mat(pkg, 0, 200, None), D=mat(pkg, 0, 17, None)))
        reaches_the_device_check(L, r(P=mat(pkg, 10, 8192, ld=128), D=mat(pkg, 10, 256, FAR), codes=(ID1,), seg=(0,) * 256, c0=0))   # 256 segments
        eight = (GOLAY, HAM3, ID1, cr.repetition(3), cr.drop(12), cr.hamming(5), cr.hamming(4), cr.identity(32))
        reaches_the_device_check(L, r(codes=eight, seg=tuple(range(8)), c0=0, D=mat(pkg, 10, sum(c.k for c in eight), FAR)))          # 8 codes
        sixteen = eight + tuple(cr.identity(n) for n in range(2, 10))
        reaches_the_device_check(L, r(codes=sixteen, seg=tuple(range(16)), c0=0, D=mat(pkg, 10, sum(c.k for c in sixteen), FAR)))      # 16 codes
        reaches_the_device_check(L, r(codes=(REP13,) * 4, seg=(0, 1, 2, 3), D=mat(pkg, 10, 4, FAR)))                                  # 16384 table words


def test_overlaps_are_refused_last(pkg, L):
    P = mat(pkg, 10, 200, BASE, 6)
    D = mat(pkg, 10, 17, FAR, 2)
    r = lambda **kw: reduce(L, pkg, **dict(dict(P=P, D=D), **kw))  # noqa: E731
    end = lambda at, ld, w: at + 8 * (9 * ld + w)   # noqa: E731  the first byte behind the last word of a 10-row matrix
    # D and P: no in-place call
    refused(L, r(D=mat(pkg, 10, 17, BASE, 6)), "overlap", "D", "P")
    refused(L, r(D=mat(pkg, 10, 17, BASE + 8 * 3, 6)), "overlap", "D", "P")                  # a word of every row
    refused(L, r(D=mat(pkg, 10, 17, BASE - 8 * 6 * 9, 6)), "overlap", "D", "P")              # its last row is P's first
    refused(L, r(D=mat(pkg, 10, 17, BASE + 8, 8)), "overlap", "D", "P")                      # another ld: address ranges
    # dist against both, pad words included
    for mname, m0, ld, w in (("P", BASE, 6, 4), ("D", FAR, 2, 1)):
        for at in (m0, m0 + 8 * ld + 8, end(m0, ld, w) - 4, m0 - 40 + 4, m0 + 8 * (ld - 1)):
            refused(L, r(dist=at), "overlap", "dist", mname)
    # a table against D and dist
    for at in (FAR, FAR + 16 + 8, end(FAR, 2, 1) - 4, FAR - 4 * 2048 + 4):
        refused(L, r(tables=[at, TAB, None]), "overlap", "leaders[0]", "D")
    refused(L, r(tables=[TAB, FAR + 8, None]), "overlap", "leaders[1]", "D")
    refused(L, r(tables=[DIST, TAB, None]), "overlap", "leaders[0]", "dist")
    refused(L, r(tables=[TAB, DIST + 36, None]), "overlap", "leaders[1]", "dist")
    refused(L, r(tables=[DIST - 4 * 2048 + 4, TAB, None]), "overlap", "leaders[0]", "dist")
    # bad arguments are reported before the overlap
    refused(L, r(D=mat(pkg, 10, 16, BASE, 6)), "D->ncols must equal K")
    refused(L, r(D=mat(pkg, 10, 17, BASE, 6), c0=190), "outside P")
    refused(L, r(D=mat(pkg, 10, 17, BASE, 6), seg=(0, 1, 7)), "seg_code[2]")
    refused(L, r(dist=BASE, tables=[TAB, None, None]), "leaders[1] is null")
    refused(L, r(dist=BASE + 2), "dist is not 4-byte aligned")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, r(D=mat(pkg, 10, 17, BASE + 8 * 6 * 10, 6)))             # right behind
        reaches_the_device_check(L, r(D=mat(pkg, 10, 17, BASE + 8 * 4, 6)))                  # in the pad words of P's rows: shares no word
        for m0, ld, w in ((BASE, 6, 4), (FAR, 2, 1)):
            reaches_the_device_check(L, r(dist=m0 - 40))                                     # right before, right behind
            reaches_the_device_check(L, r(dist=end(m0, ld, w)))
        reaches_the_device_check(L, r(tables=[FAR - 4 * 2048, end(FAR, 2, 1), None]))
        reaches_the_device_check(L, r(tables=[DIST - 4 * 2048, DIST + 40, None]))
        reaches_the_device_check(L, r(tables=[BASE, BASE + 4 * 2048, None]))                 # a table inside P: both are only read
        reaches_the_device_check(L, r(tables=[TAB, TAB, None]))                              # two codes, one table
        reaches_the_device_check(L, r(dist=None, tables=[TAB, TAB + 4 * 2048, FAR]))         # a null dist meets nothing; identity's entry is not read


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, pkg, nrows, p_ncols, codes, seg):
    out = (ctypes.c_longlong * 8)(*([-7] * 8))
    sa = (ctypes.c_ubyte * max(len(seg), 1))(*seg)
    return L.gf2_cover_plan(nrows, p_ncols, code_array(pkg, codes), len(codes), sa, len(seg), out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    to_dev = lambda c: device.CoverCode.from_rows(c.n, c.k, c.h)  # noqa: E731
    nrows = 100003
    codes = (GOLAY, HAM3, ID1, cr.identity(32))
    seen = set()
    for words in (1, 2, 3, 4, 5, 64, 65):
        ncols = 64 * words - 3
        lists = [(), (2,), (0, 1, 2), (0,) * 2 + (2,)]
        lists += [(3,) * min((ncols // 32), 256)]                                    # as many bits of the row as segments can hold
        lists += [(0,) * 10 + (2,)] if ncols >= 231 else []
        for seg in lists:
            v, o = plan(L, pkg, nrows, ncols, codes, seg)
            threads, lds, rows, lanes, K, bits, table_words, groups = o
            assert K == sum(codes[c].k for c in seg) and bits == sum(codes[c].n for c in seg) and table_words == 2048 + 8
            span = min(words, (bits + 62) // 64 + 1) if bits else 0                  # the words a window of that length can touch
            assert v == (1 if 1 <= span <= 8 else 0), (words, seg, o)
            assert threads in (64, 128, 256, 512, 1024) and rows == threads
            assert lanes == (1 if v == 0 else 1 << (span - 1).bit_length()) and lanes >= (span if v else 1)
            assert lds >= 4 * table_words + (8 * rows * span if v else 0) and lds <= 160 * 1024
            assert 1 <= groups <= (nrows + rows - 1) // rows
            # the wrapper passes the codes that the segments use, each once, in the order of their first use
            used = list(dict.fromkeys(seg))
            v2, o2 = plan(L, pkg, nrows, ncols, [codes[c] for c in used], [used.index(c) for c in seg])
            assert device.cover_plan(nrows, ncols, [to_dev(codes[c]) for c in seg]) == (v2,) + tuple(o2)
            assert (v2, o2[0], o2[2], o2[3], o2[4], o2[5], o2[7]) == (v, threads, rows, lanes, K, bits, groups) and o2[1] <= lds
            seen.add(v)
        assert plan(L, pkg, nrows, ncols, codes, (3,) * (ncols // 32 + 1))[0] == -1      # a window longer than the row
    assert seen == {0, 1}
    # the most LDS the contract allows still fits
    v, o = plan(L, pkg, 10, 512, (REP13,) * 4, (0, 1, 2, 3) * 9)
    assert v == 1 and o[6] == 16384 and 65536 < o[1] <= 160 * 1024
    assert plan(L, pkg, 0, 256, codes, (0, 1))[1][7] == 0 and plan(L, pkg, 1, 256, codes, (0, 1))[1][7] == 1
    for bad in ((-1, 256, codes, (0,)), (10, -1, codes, ()), (10, 256, codes, (4,)), (10, 256, (REP13,) * 5, (0,)), (10, 256, (), (0,)),
                (10, 256, (GOLAY,) * 17, (0,)), (10, 256, codes, (0,) * 257), (10, 22, codes, (0,))):
        assert plan(L, pkg, *bad) == (-1, [-7] * 8), bad
    assert device.cover_plan(10, 22, [device.CoverCode.golay23()]) is None
    assert device.cover_plan(10, 8192, [device.CoverCode.identity(1)] * 257) is None
    assert L.gf2_cover_plan(10, 256, code_array(pkg, codes), 4, None, 0, None) == 0     # out may be NULL; no segment: nothing to stage
