"""CPU tests of the contract of include/m4ri_hip_wht.h (gf2_lpn_tally_dev, gf2_wht_dev, gf2_lpn_errors_dev, gf2_min_weight_dev,
gf2_wht_plan): every argument is checked before a device is required and before the first HIP call, so this runs without one, on
DMatStructs around addresses that are never dereferenced (the BASE / FAR technique of tests/test_weight_contract.py).

The rule of tests/test_host_abi.py::test_header_symbols_are_exported is restated here for this companion header, because its own
list is closed: every gf2_* the header declares is exported, and the binding's table for this header (_lib.WHT_SYMBOLS) names exactly
those."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_wht.h")

BASE = 1 << 20   # an address that is never dereferenced
FAR = 1 << 28    # a second buffer, far from the first
IDX = 1 << 30    # where the index of the minimum would be
VAL = (1 << 30) + (1 << 20)
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

TALLY, WHT, ERRORS, MIN, PLAN = "gf2_lpn_tally_dev", "gf2_wht_dev", "gf2_lpn_errors_dev", "gf2_min_weight_dev", "gf2_wht_plan"
MATRIX_ENTRIES = (TALLY, ERRORS)
OUT_NAME = {TALLY: "f", ERRORS: "errors"}


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


def call(L, name, P, c0=37, k=20, label=3, out=FAR):
    return getattr(L, name)(ref(P), c0, k, label, out, None)


def minimum(L, w=BASE, n=100, idx=IDX, val=VAL):
    return L.gf2_min_weight_dev(w, n, idx, val, None)


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
    src.write_text('#include "m4ri_hip_wht.h"\nint main(void){ gf2_dmat d; long long o[12]; (void)d; return gf2_wht_plan(31, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {TALLY, WHT, ERRORS, MIN, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.WHT_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS):   # those lists stay what they were
        assert not declared & set(table)


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("OVERWRITTEN", "no host synchronisation and no hipMalloc", "has been written by the same call", "never read",
                  "at most two words", "one inside the index range included", "64-bit offsets", "Nothing of P is written",
                  "do not depend on launch order", "unsigned arithmetic", "never wrap", "modulo 2^32", "LOWEST index",
                  "nrows == 0: the tally gives zeros", "k == 0: an array of one element", "checked last", '"overlap"',
                  "before a device is required and before the first HIP call", "no other scratch", "without a device"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MATRIX_ENTRIES)
def test_argument_errors(pkg, L, name):
    P = mat(pkg, 10, 200)
    o = OUT_NAME[name]
    refused(L, call(L, name, None), name, "P is null")
    refused(L, call(L, name, mat(pkg, 10, 200, None)), name, "P.data is null")
    refused(L, call(L, name, P, out=None), name, o + " is null")
    refused(L, call(L, name, mat(pkg, -1, 200)), name, "negative")
    refused(L, call(L, name, mat(pkg, 10, -200)), name, "negative")
    refused(L, call(L, name, mat(pkg, 10, 200, ld=width(200) - 1)), name, "P.ld is smaller")
    refused(L, call(L, name, mat(pkg, 10, 200, BASE + 4)), name, "P.data is not 8-byte aligned")
    refused(L, call(L, name, P, out=FAR + 2), name, o + " is not 4-byte aligned")
    for k in (-1, 31, 1 << 20):
        refused(L, call(L, name, mat(pkg, 10, 1 << 21), k=k), name, "k = %d is outside 0 <= k <= 30" % k)
    # the column range and the label lie inside P
    refused(L, call(L, name, P, c0=-1), name, "c0", "outside P")
    refused(L, call(L, name, P, c0=181, k=20), name, "c0", "outside P")
    refused(L, call(L, name, P, c0=200, k=1), name, "c0", "outside P")
    refused(L, call(L, name, P, c0=(1 << 31) - 1, k=30), name, "c0", "outside P")
    refused(L, call(L, name, P, label=200), name, "label_col", "outside P")
    refused(L, call(L, name, P, label=-2), name, "label_col", "outside P")
    if name == ERRORS:
        refused(L, call(L, name, P, label=-1), name, "label_col", "required")
    assert L.gf2_last_error().decode().startswith(name)
    if L.gf2_device_count() <= 0:
        # rows that are only 8-byte aligned are part of the contract: an odd ld at an odd word is no argument error
        reaches_the_device_check(L, call(L, name, mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))
        reaches_the_device_check(L, call(L, name, P, out=FAR + 16))
        reaches_the_device_check(L, call(L, name, P, c0=180, k=20))            # up to the last column
        reaches_the_device_check(L, call(L, name, P, c0=50, k=30, label=199))  # over a word boundary
        reaches_the_device_check(L, call(L, name, P, c0=37, k=20, label=40))   # the label inside the index range
        reaches_the_device_check(L, call(L, name, P, c0=200, k=0))             # no index bit at all
        reaches_the_device_check(L, call(L, name, P, k=30))


def test_what_only_one_entry_refuses_or_accepts(pkg, L):
    P = mat(pkg, 10, 200)
    # the transform moves 16 bytes per access; the tally has no such need
    refused(L, call(L, ERRORS, P, out=FAR + 4), ERRORS, "errors is not 16-byte aligned")
    refused(L, call(L, ERRORS, P, k=2, out=FAR + 8), ERRORS, "errors is not 16-byte aligned")
    refused(L, L.gf2_wht_dev(FAR + 4, 2, None), WHT, "f is not 16-byte aligned")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, call(L, TALLY, P, out=FAR + 4))
        reaches_the_device_check(L, call(L, TALLY, P, label=-1))      # the plain histogram
        reaches_the_device_check(L, call(L, ERRORS, P, k=1, out=FAR + 4))
        reaches_the_device_check(L, L.gf2_wht_dev(FAR + 4, 1, None))


def test_transform_argument_errors(L):
    refused(L, L.gf2_wht_dev(None, 5, None), WHT, "f is null")
    refused(L, L.gf2_wht_dev(FAR + 2, 5, None), WHT, "f is not 4-byte aligned")
    refused(L, L.gf2_wht_dev(FAR, -1, None), WHT, "k = -1 is outside")
    refused(L, L.gf2_wht_dev(FAR, 31, None), WHT, "k = 31 is outside")
    refused(L, L.gf2_wht_dev(None, 0, None), WHT, "f is null")
    assert L.gf2_last_error().decode().startswith(WHT)
    assert L.gf2_wht_dev(FAR + 4, 0, None) == 0     # k == 0: the identity, no device needed
    if L.gf2_device_count() <= 0:
        for k in (1, 2, 12, 13, 30):
            reaches_the_device_check(L, L.gf2_wht_dev(FAR, k, None))


@pytest.mark.parametrize("name", MATRIX_ENTRIES)
def test_an_output_inside_the_operand_is_refused(pkg, L, name):
    P = mat(pkg, 10, 200, FAR, 6)
    k = 4
    nbytes = 4 << k
    last = FAR + 8 * (9 * 6 + width(200))   # the first byte behind P's last word
    assert last % 16 == 0
    for out in (FAR, FAR + 8 * 6 + 8 + 8, last - 16, FAR - nbytes + 16):
        refused(L, call(L, name, P, c0=0, k=k, out=out), name, "overlap", OUT_NAME[name], "P")
    # the pad words between the rows belong to P's address range
    refused(L, call(L, name, P, c0=0, k=0, out=FAR + 8 * 4), name, "overlap")
    # bad arguments are reported before the overlap
    refused(L, call(L, name, P, c0=0, k=31, out=FAR), name, "k = 31")
    refused(L, call(L, name, P, c0=0, k=k, label=200, out=FAR), name, "label_col")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, call(L, name, P, c0=0, k=k, out=FAR - nbytes))   # right before
        reaches_the_device_check(L, call(L, name, P, c0=0, k=k, out=last))           # right behind


def test_empty_shapes(pkg, L):
    # no rows: the answer is zeros, which still needs the device; data may be null, nothing is read
    refused(L, call(L, TALLY, mat(pkg, 0, 200, None), out=None), TALLY, "f is null")
    refused(L, call(L, TALLY, mat(pkg, 0, 0, None), c0=0, k=1, label=-1), TALLY, "outside P")
    refused(L, call(L, ERRORS, mat(pkg, 5, 0, None), c0=0, k=0, label=0), ERRORS, "label_col")
    if L.gf2_device_count() <= 0:
        for name in MATRIX_ENTRIES:
            reaches_the_device_check(L, call(L, name, mat(pkg, 0, 200, None)))
            reaches_the_device_check(L, call(L, name, mat(pkg, 0, 200, None), c0=0, k=0))
            reaches_the_device_check(L, call(L, name, mat(pkg, 10, 200), c0=5, k=0))
        reaches_the_device_check(L, call(L, TALLY, mat(pkg, 0, 0, None), c0=0, k=0, label=-1))
        reaches_the_device_check(L, call(L, TALLY, mat(pkg, 7, 0, None), c0=0, k=0, label=-1))   # f[0] = 7: no bit of P is read


def test_min_argument_errors_and_aliasing(L):
    refused(L, minimum(L, n=0), MIN, "n = 0 is below 1")
    refused(L, minimum(L, n=-5), MIN, "below 1")
    refused(L, minimum(L, w=None), MIN, "w is null")
    refused(L, minimum(L, idx=None), MIN, "idx is null")
    refused(L, minimum(L, val=None), MIN, "val is null")
    refused(L, minimum(L, w=BASE + 2), MIN, "w is not 4-byte aligned")
    refused(L, minimum(L, idx=IDX + 1), MIN, "idx is not 4-byte aligned")
    refused(L, minimum(L, val=VAL + 2), MIN, "val is not 4-byte aligned")
    assert L.gf2_last_error().decode().startswith(MIN)
    n = 100
    for p in (BASE, BASE + 4 * (n - 1)):
        refused(L, minimum(L, n=n, idx=p), MIN, "overlap", "idx", "w")
        refused(L, minimum(L, n=n, val=p), MIN, "overlap", "val", "w")
    refused(L, minimum(L, idx=IDX, val=IDX), MIN, "overlap", "idx", "val")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, minimum(L))
        reaches_the_device_check(L, minimum(L, n=1))
        reaches_the_device_check(L, minimum(L, w=BASE + 4, n=(1 << 31) - 1, idx=BASE, val=BASE - 4))   # right before
        reaches_the_device_check(L, minimum(L, n=n, idx=BASE + 4 * n, val=BASE + 4 * n + 4))         # right behind, side by side


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, k):
    out = (ctypes.c_longlong * 12)(*([-7] * 12))
    return L.gf2_wht_plan(k, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    variants, counts = [], []
    for k in range(31):
        passes, o = plan(L, k)
        first, threads, lds, variant, scratch = o[:8], o[8], o[9], o[10], o[11]
        assert (passes == 0) == (k == 0) and 0 <= passes <= 8, (k, passes)
        # the passes partition [0, k) in ascending order: no level twice, none missing
        bounds = first[:passes] + [k]
        assert bounds[0] == (0 if k else k) and all(a < b for a, b in zip(bounds, bounds[1:])), (k, o)
        assert all(x == k for x in first[passes:]), (k, o)
        levels = [l for a, b in zip(bounds, bounds[1:]) for l in range(a, b)]
        assert levels == list(range(k)), (k, o)
        assert 0 <= lds <= 160 * 1024 and threads in (64, 128, 256, 512, 1024), (k, o)
        assert variant in (0, 1) and 8 <= scratch <= 8 << 20 and scratch % 8 == 0, (k, o)
        variants.append(variant)
        counts.append(passes)
        assert device.wht_plan(k) == (passes, bounds, threads, lds, variant, scratch)
    assert sum(a != b for a, b in zip(variants, variants[1:])) == 1 and variants[0] == 0 and variants[-1] == 1
    assert counts == sorted(counts)   # more levels never take fewer passes
    for k in (-1, 31):
        assert plan(L, k)[0] == -1 and plan(L, k)[1] == [-7] * 12
        assert device.wht_plan(k) is None
    assert L.gf2_wht_plan(20, None) == plan(L, 20)[0] and L.gf2_wht_plan(0, None) == 0 and L.gf2_wht_plan(31, None) == -1
