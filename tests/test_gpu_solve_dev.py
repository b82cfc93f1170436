"""GPU tests of gf2_solve_left_dev (device.solve_left): mzd_solve_left's contract on device matrices.  Every case checks, against the
oracle (gf2util.o_solve_left, o_echelonize): all B.nrows rows of B after the call (X, then zero rows), A holding its reduced row
echelon form, the inconsistency flag, and the excess bits of both last words."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest

import gf2util as g
import ple_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


@pytest.fixture(scope="module")
def dev(pkg):
    from m4ri_rust_amd import device
    return device


def no_excess(words, ncols):
    return ncols % 64 == 0 or not (words[:, -1] >> np.uint64(ncols % 64)).any()


def raw_solve(pkg, A, B, check):
    bad = ctypes.c_int(-1)
    rc = pkg._lib.lib().gf2_solve_left_dev(ctypes.byref(A.s), ctypes.byref(B.s), check, ctypes.byref(bad), None)
    return rc, bad.value


def solve_and_check(pkg, dev, a, m, n, b, brows, k, check=1):
    """b: brows x width(k) words (right-hand side in the first m rows, anything below) -> consistent? by the oracle"""
    want_x, consistent = g.o_solve_left(a, m, n, b, brows, k)
    red = g.o_echelonize(a, m, n, full=True)[0]
    A, B = dev.DMat.from_words(a, n), dev.DMat.from_words(b, k)
    rc, bad = raw_solve(pkg, A, B, check)
    assert rc == 0, pkg._lib.lib().gf2_last_error()
    assert bad == (0 if consistent or not check else 1)
    x, ra = B.to_words(), A.to_words()
    assert x.shape == (brows, g.width(k))
    assert np.array_equal(x, want_x), "B: the solution rows, then zero rows"
    assert not x[n:].any()
    assert np.array_equal(ra, red), "A does not hold its reduced echelon form"
    assert no_excess(x, k) and no_excess(ra, n)
    if consistent:
        assert np.array_equal(g.o_mul_naive(np.ascontiguousarray(a), np.ascontiguousarray(x[:n]), m, n, k), b[:m]), "A X != B"
    return consistent


@functools.lru_cache(maxsize=None)
def full_rank(m, n, seed):
    """a random m x n matrix of rank min(m, n): the first seed from `seed` on that gives one"""
    while True:
        a = g.random_words(m, n, seed)
        if g.o_echelonize(a, m, n)[1] == min(m, n):
            a.setflags(write=False)
            return a
        seed += 1000


def rhs(a, m, n, k, brows, seed):
    """B = A X0 through the oracle product in the first m rows, random bits below"""
    b = g.random_words(brows, k, seed + 1)
    b[:m] = g.o_mul_naive(np.ascontiguousarray(a), g.random_words(n, k, seed), m, n, k)
    return b


@pytest.mark.parametrize("name", ["solve_120x80x33", "solve_lowrank_200x150x70_r40"])
def test_fixtures(pkg, dev, name):
    d = np.load(os.path.join(HERE, "golden", "elim", name + ".npz"))
    m, n, k = (int(x) for x in d["shape"])
    A, B = dev.DMat.from_words(d["a"], n), dev.DMat.from_words(d["b"], k)
    assert dev.solve_left(A, B) is True
    assert np.array_equal(B.to_words(), d["x"])
    assert solve_and_check(pkg, dev, d["a"], m, n, d["b"], max(m, n), k) is True
    assert solve_and_check(pkg, dev, d["a"], m, n, d["b_inconsistent"], max(m, n), k) is (not bool(d["inconsistent"][0]))


@pytest.mark.parametrize("m,n,k", [(64, 64, 1), (65, 63, 64), (63, 65, 65), (130, 70, 129), (1, 1, 1)])
def test_full_rank(pkg, dev, m, n, k):
    a = full_rank(m, n, 100 * m + n)
    assert solve_and_check(pkg, dev, a, m, n, rhs(a, m, n, k, max(m, n), 7), max(m, n), k) is True


@pytest.mark.parametrize("m,n,r,k", [(200, 150, 40, 70), (300, 400, 37, 5)])
def test_rank_deficient(pkg, dev, m, n, r, k):
    a = ple_cases.low_rank(m, n, r, 11 * m + n)
    brows = max(m, n)
    b = rhs(a, m, n, k, brows, 9)
    assert solve_and_check(pkg, dev, a, m, n, b, brows, k) is True
    # a dependent row by the oracle's elimination of [A | I]: a row of the transformation below the rank combines rows of A to zero;
    # flipping one bit of B in the LAST row that takes part makes the same combination of B non-zero
    t = np.zeros((m, g.width(n) * 64 + m), dtype=np.uint8)
    t[:, :n] = g.words_to_bits(a, n)
    t[:, g.width(n) * 64:] = np.eye(m, dtype=np.uint8)
    red, rank, _ = g.o_echelonize(g.bits_to_words(t), m, t.shape[1], full=True, limit=n)
    assert rank < m
    combo = g.words_to_bits(red, t.shape[1])[rank, g.width(n) * 64:]
    row = int(np.flatnonzero(combo)[-1])
    b2 = b.copy()
    b2[row, 0] ^= np.uint64(1)
    assert solve_and_check(pkg, dev, a, m, n, b2, brows, k, check=1) is False
    assert solve_and_check(pkg, dev, a, m, n, b2, brows, k, check=0) is False  # same return code, the flag stays 0


def test_surplus_rows_of_b_come_back_zero(pkg, dev):
    m, n, k, brows = 65, 63, 64, 100
    a = full_rank(m, n, 100 * m + n)
    assert solve_and_check(pkg, dev, a, m, n, rhs(a, m, n, k, brows, 21), brows, k) is True
    m, n, k, brows = 63, 65, 65, 90
    a = full_rank(m, n, 100 * m + n)
    assert solve_and_check(pkg, dev, a, m, n, rhs(a, m, n, k, brows, 22), brows, k) is True


@pytest.mark.parametrize("m,n,k", [(192, 256, 64), (193, 257, 64), (600, 520, 130)], ids=["single_launch", "blocked", "blocked_m_gt_n"])
def test_both_sides_of_the_small_elimination(pkg, dev, m, n, k):
    """gf2_echelonize_dev takes its single-launch path while at most 256 columns can matter (min(n, m + 64) <= 256, and the matrix fits
    into LDS): [A | B] of 192 x 256 is the last shape that does, 193 x 257 the first that takes the blocked path"""
    a = full_rank(m, n, 100 * m + n)
    assert solve_and_check(pkg, dev, a, m, n, rhs(a, m, n, k, max(m, n), 31), max(m, n), k) is True


def dirty(nrows, ld, seed):
    return g.splitmix64(seed, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld)


@pytest.mark.parametrize("consistent", [True, False])
def test_strided_views_of_dirty_buffers(pkg, dev, consistent):
    """A and B as offset, strided views (16-byte aligned, even ld, as a gf2_dmat asks) of buffers full of random bits"""
    import torch
    m, n, r, k, brows = 200, 150, 40, 70, 210
    a = ple_cases.low_rank(m, n, r, 41)
    b = rhs(a, m, n, k, brows, 42) if consistent else g.random_words(brows, k, 43)
    (ald, ar0, acw0, aprows), (bld, br0, bcw0, bprows) = (10, 3, 4, 205), (6, 2, 2, 215)
    ahost, bhost = dirty(aprows, ald, 44), dirty(bprows, bld, 45)
    ahost[ar0:ar0 + m, acw0:acw0 + g.width(n)] = a
    bhost[br0:br0 + brows, bcw0:bcw0 + g.width(k)] = b
    ta = torch.from_numpy(ahost.view(np.int64).copy()).cuda()
    tb = torch.from_numpy(bhost.view(np.int64).copy()).cuda()
    A = dev.DMat.wrap(ta.data_ptr() + 8 * (ar0 * ald + acw0), m, n, ald, keep=ta)
    B = dev.DMat.wrap(tb.data_ptr() + 8 * (br0 * bld + bcw0), brows, k, bld, keep=tb)
    want_x, ok = g.o_solve_left(a, m, n, b, brows, k)
    assert ok is consistent
    assert dev.solve_left(A, B) is consistent
    torch.cuda.synchronize()
    ea, eb = ahost.copy(), bhost.copy()
    ea[ar0:ar0 + m, acw0:acw0 + g.width(n)] = g.o_echelonize(a, m, n, full=True)[0]
    eb[br0:br0 + brows, bcw0:bcw0 + g.width(k)] = want_x
    assert np.array_equal(ta.cpu().numpy().view(np.uint64), ea), "A's view, or its parent outside the view"
    assert np.array_equal(tb.cpu().numpy().view(np.uint64), eb), "B's view, or its parent outside the view"


def test_same_answer_as_the_friendly_layer(pkg, dev):
    """device.solve_left against friendly.solve_left (mzd_solve_left, on the device too: the suite switches the size dispatch off)"""
    assert os.environ.get("M4RI_HIP_HOST_SMALL_WORK") == "0"
    for m, n, r, k, consistent in ((200, 150, 40, 70, True), (200, 150, 40, 70, False), (130, 70, 70, 129, True)):
        a = ple_cases.low_rank(m, n, r, 51) if r < min(m, n) else full_rank(m, n, 100 * m + n)
        brows = max(m, n)
        b = rhs(a, m, n, k, brows, 52) if consistent else g.random_words(brows, k, 53)
        HA, HB = pkg.BinMatrix.from_words(a, n), pkg.BinMatrix.from_words(b, k)
        DA, DB = dev.DMat.from_words(a, n), dev.DMat.from_words(b, k)
        flag = pkg.solve_left(HA, HB)
        assert dev.solve_left(DA, DB) is flag is consistent
        assert np.array_equal(DB.to_words(), HB.to_words())
        assert np.array_equal(DA.to_words(), HA.to_words())


def test_nothing_to_do_and_shape_errors(pkg, dev):
    L = pkg._lib.lib()
    a, b = g.random_words(5, 7, 61), g.random_words(9, 3, 62)
    A, B = dev.DMat.from_words(a, 7), dev.DMat.from_words(b, 3)
    empty = pkg._lib.DMatStruct(None, 0, 5, 0)
    bad = ctypes.c_int(-1)
    assert L.gf2_solve_left_dev(ctypes.byref(empty), ctypes.byref(B.s), 1, ctypes.byref(bad), None) == 0 and bad.value == 0
    assert np.array_equal(B.to_words(), b)
    small = dev.DMat.from_words(g.random_words(6, 3, 63), 3)
    assert L.gf2_solve_left_dev(ctypes.byref(A.s), ctypes.byref(small.s), 1, ctypes.byref(bad), None) == -1
    assert b"B.nrows" in L.gf2_last_error()
    with pytest.raises(pkg._lib.HipError):
        dev.solve_left(A, small)
    assert np.array_equal(A.to_words(), a)
