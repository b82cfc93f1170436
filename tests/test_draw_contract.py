"""CPU tests of the contract of include/m4ri_hip_draw.h (gf2_bernoulli_dev, gf2_bernoulli_block_dev, gf2_draw_indices_dev,
gf2_draw_subsets_dev, gf2_draw_permutation_dev, gf2_draw_plan): every argument is checked before a device is required and before the
first HIP call, so this runs without one, on addresses that are never dereferenced (the BASE / FAR technique of
tests/test_lf2_contract.py).

Every gf2_* the header declares is exported, and the binding's table for this header (_lib.DRAW_SYMBOLS) names exactly those; the
tables of the older headers do not."""
import ctypes
import os
import re
import subprocess

import pytest

import draw_ref as dr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "m4ri_hip_draw.h")

BASE = 1 << 20     # D: an address that is never dereferenced
IDX = 1 << 28      # idx, sub, perm
UNF = 1 << 29      # unfinished
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

BERN, BLOCK, INDICES, SUBSETS, PERM, PLAN = ("gf2_bernoulli_dev", "gf2_bernoulli_block_dev", "gf2_draw_indices_dev", "gf2_draw_subsets_dev",
                                             "gf2_draw_permutation_dev", "gf2_draw_plan")


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


def bern(L, name, D, thr=0x20000000, seed=1, accumulate=0, row0=0, col_word0=0, full_ncols=0):
    if name == BERN:
        return L.gf2_bernoulli_dev(ref(D), thr, seed, accumulate, None)
    return L.gf2_bernoulli_block_dev(ref(D), thr, seed, row0, col_word0, full_ncols, accumulate, None)


def indices(L, idx=IDX, count=10, n=100):
    return L.gf2_draw_indices_dev(idx, count, n, 1, None)


def subsets(L, sub=IDX, batch=10, k=8, n=100, max_rounds=0, unfinished=UNF):
    return L.gf2_draw_subsets_dev(sub, batch, k, n, 1, max_rounds, unfinished, None)


def perm(L, p=IDX, n=10):
    return L.gf2_draw_permutation_dev(p, n, 1, None)


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in words), msg
    assert msg.startswith(words[0]), msg


def reaches_the_device_check(L, rc):
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def declarations():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gf2_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_compiles_as_c11(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "m4ri_hip_draw.h"\nint main(void){ gf2_dmat d; long long o[4]; (void)d; '
                   'return gf2_draw_plan(GF2_DRAW_SUBSETS, 2000, 10, 0, o) != -1; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_header_symbols_are_exported(pkg):
    declared = set(declarations())
    assert declared == {BERN, BLOCK, INDICES, SUBSETS, PERM, PLAN}
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert declared <= exported, sorted(declared - exported)
    assert declared == set(pkg._lib.DRAW_SYMBOLS)
    for table in (pkg._lib.DECLARED_SYMBOLS, pkg._lib.GATHER_SYMBOLS, pkg._lib.WEIGHT_SYMBOLS, pkg._lib.WHT_SYMBOLS, pkg._lib.BKW_SYMBOLS,
                  pkg._lib.COVER_SYMBOLS, pkg._lib.LF2_SYMBOLS):   # stay what they were
        assert not declared & set(table)
    assert set(pkg._lib.LF2_SYMBOLS) == {"gf2_class_sort_dev", "gf2_lf2_reduce_dev", "gf2_lf2_plan"}


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"(?m)^ \* ?", "", open(HEADER).read()).split())   # the comment without its line starts
    for words in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "ten rounds", "(seed low 32, seed high 32)",
                  "1 Bernoulli, 2 indices, 3 subsets, 4 permutation", "mulhi64(X, n)", "a bias below n / 2^64",
                  "a function of (seed, thr, word index, bit) only", "widx = (row0 + r) * fullw + col_word0 + j", "U_i < thr",
                  "q = ctz(thr) / 2 .. 15", "thr == 0 makes no call", "by the rule of gf2_submatrix_dev", "D is never read",
                  "excess bits stay as they were", "16-byte stores are used only where every row allows it", "64-bit offsets",
                  "WITH replacement", "count == 0: nothing is written", "DISTINCT", "1 <= k <= 1024 and 2 k <= n",
                  "max_rounds == 0 means 64", "read -1", "OVERWRITTEN with the number of subsets", "bounded in time by construction",
                  "in (round, position) order", "STABLE argsort", "Ties fall in index order", "below n^2 / 2^31 in total variation",
                  "n == 0: nothing is written", "no host synchronisation and no hipMalloc", "has been written by the same call",
                  "Two runs give the same bits", "before a device is required and before the first HIP call", "checked last", '"overlap"',
                  "without a device"):
        assert words in text, words


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [BERN, BLOCK])
def test_bernoulli_argument_errors(pkg, L, name):
    c = lambda D, **kw: bern(L, name, D, **kw)  # noqa: E731
    refused(L, c(None), name, "D is null")
    refused(L, c(mat(pkg, 10, 200, None)), name, "D.data is null")
    refused(L, c(mat(pkg, -1, 200)), name, "negative")
    refused(L, c(mat(pkg, 10, -200)), name, "negative")
    refused(L, c(mat(pkg, 10, 200, ld=width(200) - 1)), name, "D.ld is smaller")
    refused(L, c(mat(pkg, 10, 200, BASE + 4)), name, "D.data is not 8-byte aligned")
    if name == BLOCK:
        D = mat(pkg, 10, 200)
        refused(L, c(D, row0=-1), name, "row0 = -1", "negative")
        refused(L, c(D, col_word0=-1), name, "col_word0 = -1", "negative")
        refused(L, c(D, full_ncols=-64), name, "full_ncols = -64", "negative")
        refused(L, c(D, col_word0=1, full_ncols=256), name, "outside the whole matrix")
        refused(L, c(D, full_ncols=192), name, "outside the whole matrix")
    if L.gf2_device_count() <= 0:
        for thr in dr_thrs():
            for acc in (0, 1):
                reaches_the_device_check(L, c(mat(pkg, 10, 200), thr=thr, accumulate=acc))
        reaches_the_device_check(L, c(mat(pkg, 10, 200, BASE + 8, ld=width(200) + 1)))   # rows that are only 8-byte aligned
        reaches_the_device_check(L, c(mat(pkg, 0, 200, None)))
        reaches_the_device_check(L, c(mat(pkg, 7, 0, None)))
        if name == BLOCK:
            reaches_the_device_check(L, c(mat(pkg, 10, 200), row0=(1 << 40), col_word0=3, full_ncols=64 * 7))
            reaches_the_device_check(L, c(mat(pkg, 10, 200), row0=5, col_word0=0, full_ncols=0))


def dr_thrs():
    return [0, 1, 0x20000000, 0x80000000, 0x12345679, 0xFFFFFFFF]


def test_indices_argument_errors(L):
    refused(L, indices(L, idx=None), INDICES, "idx is null")
    refused(L, indices(L, idx=IDX + 2), INDICES, "idx is not 4-byte aligned")
    refused(L, indices(L, count=-1), INDICES, "count = -1 is negative")
    for n in (0, -1, -(1 << 31)):
        refused(L, indices(L, n=n), INDICES, "n = %d is outside 1 <= n" % n)
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, indices(L))
        reaches_the_device_check(L, indices(L, idx=IDX + 4, count=0))
        reaches_the_device_check(L, indices(L, n=1))
        reaches_the_device_check(L, indices(L, count=1 << 40, n=(1 << 31) - 1))


def test_subsets_argument_errors(L):
    refused(L, subsets(L, sub=None), SUBSETS, "sub is null")
    refused(L, subsets(L, sub=IDX + 1), SUBSETS, "sub is not 4-byte aligned")
    refused(L, subsets(L, batch=-1), SUBSETS, "batch = -1 is negative")
    for k in (0, -1, 1025):
        refused(L, subsets(L, k=k, n=1 << 20), SUBSETS, "k = %d is outside 1 <= k <= 1024" % k)
    for n in (0, -5):
        refused(L, subsets(L, k=1, n=n), SUBSETS, "n = %d is outside 1 <= n" % n)
    for k, n in ((1, 1), (8, 15), (1024, 2047)):
        refused(L, subsets(L, k=k, n=n), SUBSETS, "2 k may not exceed n")
    for r in (-1, 65, 1 << 20):
        refused(L, subsets(L, max_rounds=r), SUBSETS, "max_rounds = %d is outside 0 <= max_rounds <= 64" % r)
    refused(L, subsets(L, unfinished=UNF + 2), SUBSETS, "unfinished is not 4-byte aligned")
    # aliasing, last: sub holds batch * k = 80 ints
    for at in (IDX, IDX + 4 * 79, IDX + 160):
        refused(L, subsets(L, unfinished=at), SUBSETS, "overlap", "sub", "unfinished")
    refused(L, subsets(L, unfinished=IDX, max_rounds=65), SUBSETS, "max_rounds")      # bad arguments before the overlap
    refused(L, subsets(L, unfinished=IDX, k=8, n=15), SUBSETS, "2 k may not exceed n")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, subsets(L))
        reaches_the_device_check(L, subsets(L, unfinished=None))
        reaches_the_device_check(L, subsets(L, unfinished=IDX + 4 * 80))      # right behind
        reaches_the_device_check(L, subsets(L, unfinished=IDX - 4))           # right before
        reaches_the_device_check(L, subsets(L, batch=0, unfinished=IDX))      # no subset: an empty array
        for k, n in ((1, 2), (8, 16), (1024, 2048), (64, (1 << 31) - 1)):
            reaches_the_device_check(L, subsets(L, k=k, n=n))
        for r in (0, 1, 64):
            reaches_the_device_check(L, subsets(L, max_rounds=r))


def test_permutation_argument_errors(L):
    refused(L, perm(L, p=None), PERM, "perm is null")
    refused(L, perm(L, p=IDX + 2), PERM, "perm is not 4-byte aligned")
    refused(L, perm(L, n=-1), PERM, "n = -1 is negative")
    if L.gf2_device_count() <= 0:
        reaches_the_device_check(L, perm(L))
        reaches_the_device_check(L, perm(L, n=0))
        reaches_the_device_check(L, perm(L, n=(1 << 31) - 1))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

def plan(L, what, count_or_k=0, n=1, thr=0):
    out = (ctypes.c_longlong * 4)(*([-7] * 4))
    return L.gf2_draw_plan(what, count_or_k, n, thr, out), [int(x) for x in out]


def test_plan(pkg, L):
    from m4ri_rust_amd import device
    B, I, S, P = pkg._lib.DRAW_BERNOULLI, pkg._lib.DRAW_INDICES, pkg._lib.DRAW_SUBSETS, pkg._lib.DRAW_PERMUTATION
    assert (B, I, S, P) == (1, 2, 3, 4)
    # the skip rule: the calls q = ctz(thr) / 2 .. 15
    for thr, calls in ((0, 0), (1, 16), (3, 16), (0x12345679, 16), (0xFFFFFFFF, 16), (2, 16), (4, 15), (8, 15), (0x20000000, 2),
                       (0x40000000, 1), (0x80000000, 1), (0x12345678, 15), (0xFFFF0000, 8)):
        rc, o = plan(L, B, thr=thr)
        assert rc == 0 and o[0] == calls == dr.bernoulli_words(0, [0], thr)[1], (hex(thr), o)
        assert o[1] in (64, 128, 256, 512, 1024) and o[2] % o[1] == 0 and o[2] >= o[1]
        assert device.draw_plan("bernoulli", thr=thr) == tuple(o)
    rc, o = plan(L, I, 1001, 5)
    assert rc == 0 and o[0] == 501 and o[2] % 2 == 0 and device.draw_plan("indices", 1001, 5) == tuple(o)
    assert plan(L, I, 0, 5)[1][0] == 0
    for bad in ((I, -1, 5), (I, 5, 0), (S, 0, 100), (S, 1025, 1 << 20), (S, 8, 15), (S, 1, 1), (P, 0, -1), (0, 1, 1), (5, 1, 1)):
        assert plan(L, *bad) == (-1, [-7] * 4), bad
        assert device.draw_plan(*bad) is None
    per_group = []
    for k in (1, 2, 8, 64, 65, 512, 1024):
        rc, o = plan(L, S, k, 2 * k)
        threads, lds, per, rounds = o
        assert rc == 0 and threads in (64, 128, 256, 512, 1024) and rounds == 64, (k, o)
        assert per >= 1 and 8 * k * per <= lds <= 160 * 1024, (k, o)           # a settled value and a draw per position
        assert (per > 1) == (k <= 64) and k <= threads * max(1, 1024 // threads), (k, o)
        assert device.draw_plan("subsets", k, 2 * k) == tuple(o)
        per_group.append(per)
    assert per_group == sorted(per_group, reverse=True)
    for n in (1, 255, 70000, 1 << 20):
        rc, o = plan(L, P, 0, n)
        assert rc == 0 and o[1] == 4 and o[2] == 30 and o[0] >= 16 * n       # two buffers of (key, i) pairs
        assert o[0] == device.lf2_plan(n, 64, 30)[7]                         # the class sort's own scratch
        assert device.draw_plan("permutation", n=n) == tuple(o)
    assert plan(L, P, 0, 0) == (0, [0, 4, 30, 0])
    assert L.gf2_draw_plan(B, 0, 1, 1, None) == 0 and L.gf2_draw_plan(S, 8, 15, 0, None) == -1
