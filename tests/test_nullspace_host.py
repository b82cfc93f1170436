"""CPU tests of gf2_nullspace_host_small, the host routine of mzd_kernel_left_pluq's size dispatch: the pattern list of
tests/nullspace_ref.py (the small shapes) and random low-rank matrices, K bit for bit against the basis read off the constructed
echelon form, A left holding the oracle's reduced echelon form, A0 K = 0; a window of a dirty parent; full column rank.  No device is
needed."""
import ctypes

import numpy as np
import pytest

import gf2util as g
import nullspace_ref as R
import ple_cases

SMALL = [p for p in R.patterns() if p[2] <= 1000]


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    return p


def run_host(pkg, A):
    """gf2_nullspace_host_small on the BinMatrix (or mzd_t pointer) A -> (K words or None, rank)"""
    L = pkg._lib.lib()
    kp = pkg._lib.MzdP()
    calls = L.gf2_host_small_calls()
    rank = L.gf2_nullspace_host_small(A.mzd if hasattr(A, "mzd") else A, ctypes.byref(kp))
    assert L.gf2_host_small_calls() == calls + 1
    return (pkg.BinMatrix(kp).to_words() if kp else None), rank


def check(pkg, a0, m, n, want_k):
    A = pkg.BinMatrix.from_words(a0, n)
    k, rank = run_host(pkg, A)
    red, orank, opiv = g.o_echelonize(a0, m, n, full=True)
    d = n - orank
    assert rank == orank
    assert np.array_equal(A.to_words(), red), "A does not hold the reduced echelon form"
    if d == 0:
        assert k is None
        return
    assert k.shape == want_k.shape and np.array_equal(k, want_k), "K differs from the basis of the contract"
    assert R.no_excess(k, d)
    assert not g.o_mul_fast(np.ascontiguousarray(a0), k, m, n, d).any(), "A0 K != 0"


@pytest.mark.parametrize("name,m,n,S", SMALL, ids=[p[0] for p in SMALL])
def test_patterns(pkg, name, m, n, S):
    a0, want = R.with_pivots(m, n, S, seed=len(name) + m + n)
    assert g.o_echelonize(a0, m, n)[2] == [int(c) for c in S]  # the construction has the pivots it was asked for
    check(pkg, a0, m, n, want)


@pytest.mark.parametrize("m,n,r", [(300, 400, 37), (70, 130, 64), (130, 70, 70), (1, 200, 1)])
def test_low_rank_through_the_oracle(pkg, m, n, r):
    a0 = ple_cases.low_rank(m, n, r, 5 * m + n)
    red, rank, piv = g.o_echelonize(a0, m, n, full=True)
    check(pkg, a0, m, n, R.from_rref(red, piv, n))


def test_full_column_rank_gives_null(pkg):
    a0 = g.random_words(200, 130, 9)
    A = pkg.BinMatrix.from_words(a0, 130)
    k, rank = run_host(pkg, A)
    assert k is None and rank == 130
    assert np.array_equal(A.to_words(), g.o_echelonize(a0, 200, 130)[0])


def test_null_arguments_are_refused(pkg):
    L = pkg._lib.lib()
    kp = pkg._lib.MzdP()
    assert L.gf2_nullspace_host_small(None, ctypes.byref(kp)) == -1
    assert L.gf2_nullspace_host_small(pkg.BinMatrix.zero(3, 3).mzd, None) == -1


@pytest.mark.parametrize("m,n,S", [(40, 130, range(0, 130, 5)), (70, 64, range(10, 60)), (20, 200, [0, 63, 64, 127, 128, 199])])
def test_window_of_a_dirty_parent(pkg, m, n, S):
    """random bits in every word of the parent, the excess bits included: only the window changes"""
    L = pkg._lib.lib()
    a0, want = R.with_pivots(m, n, S, seed=m + n)
    r0, c0 = 3, 64
    rows, cols = r0 + m + 2, c0 + n + 70
    P = pkg.BinMatrix.zero(rows, cols)
    w = g.width(cols)
    P._words_view()[:, :w] = g.splitmix64(m * n, np.arange(rows * w, dtype=np.uint64)).reshape(rows, w)
    before = g.words_to_bits(P.to_words(), w * 64)
    before[r0:r0 + m, c0:c0 + n] = g.words_to_bits(a0, n)
    P._words_view()[:, :w] = g.bits_to_words(before)
    W = L.mzd_init_window(P.mzd, r0, c0, r0 + m, c0 + n)
    k, rank = run_host(pkg, W)
    L.mzd_free(W)
    after = g.words_to_bits(P.to_words(), w * 64)
    expect = before.copy()
    expect[r0:r0 + m, c0:c0 + n] = g.words_to_bits(g.o_echelonize(a0, m, n)[0], n)
    assert np.array_equal(after, expect), "the window's reduced form, or the parent outside the window"
    assert rank == len(S) and np.array_equal(k, want)
