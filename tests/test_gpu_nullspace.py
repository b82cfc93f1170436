"""GPU tests of the null space (gf2_nullspace.hip): gf2_nullspace_dev through device.nullspace, the host entry mzd_kernel_left_pluq in
both modes of the size dispatch, BinMatrix.kernel and DMat.kernel.  Every case checks the same six things: K bit for bit against
tests/nullspace_ref.py, the excess bits of K's last word, the rank, the pivot columns, A equal to the oracle's reduced echelon form,
and A0 K = 0.  The pattern list holds the smallest shapes at which the column compress can go wrong."""
import ctypes

import numpy as np
import pytest

import gf2util as g
import nullspace_ref as R
import ple_cases
from stream_util import on_stream, padded

pytestmark = pytest.mark.gpu

PATTERNS = R.patterns()


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


@pytest.fixture(params=["device", "dispatch"])
def mode(request, monkeypatch):
    if request.param == "dispatch":
        monkeypatch.delenv("M4RI_HIP_HOST_SMALL_WORK", raising=False)  # the library default
    else:
        monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", "0")
    return request.param


def six_checks(a0, m, n, got_k, rank, piv, got_a, want_k):
    """got_k: K's words as stored (None: no basis), got_a: what A holds after the call"""
    red, orank, opiv = g.o_echelonize(a0, m, n, full=True)
    d = n - orank
    assert rank == orank
    assert list(piv) == opiv
    assert np.array_equal(got_a, red), "A does not hold the reduced echelon form"
    if d == 0:
        assert got_k is None
        return
    assert got_k is not None and got_k.shape == (n, g.width(d))
    assert R.no_excess(got_k, d), "excess bits of K's last word"
    assert np.array_equal(got_k, want_k), "K differs from the basis of the contract"
    assert not g.o_mul_fast(np.ascontiguousarray(a0), got_k, m, n, d).any(), "A0 K != 0"


def run_dev(a0, m, n, want_k):
    from m4ri_rust_amd import device
    A = device.DMat.from_words(a0, n)
    K, rank, piv = device.nullspace(A)
    if K is not None:
        assert (K.nrows, K.ncols) == (n, n - rank) and K.ld >= g.width(n - rank)
    six_checks(a0, m, n, None if K is None else K.to_words(), rank, piv, A.to_words(), want_k)
    return K


@pytest.mark.parametrize("name,m,n,S", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_patterns(pkg, name, m, n, S):
    a0, want = R.with_pivots(m, n, S, seed=len(name) + m + n)
    K = run_dev(a0, m, n, want)
    assert (K is None) == (len(S) == n)


@pytest.mark.parametrize("m,n,r", [(300, 400, 37), (1100, 2300, 1000)])
def test_random_low_rank(pkg, m, n, r):
    a0 = ple_cases.low_rank(m, n, r, 3 * m + n)
    red, rank, piv = g.o_echelonize(a0, m, n, full=True)
    run_dev(a0, m, n, R.from_rref(red, piv, n))


def test_full_column_rank(pkg):
    """no basis: K = {NULL, 0, n, 0}, and mzd_kernel_left_pluq returns NULL"""
    from m4ri_rust_amd import device
    L = pkg._lib.lib()
    m, n = 200, 130
    a0 = g.random_words(m, n, 9)
    A = device.DMat.from_words(a0, n)
    ks = pkg._lib.DMatStruct(1, 7, 7, 7)
    rank = ctypes.c_int(-1)
    assert L.gf2_nullspace_dev(ctypes.byref(A.s), ctypes.byref(ks), ctypes.byref(rank), None, None) == 0
    assert rank.value == n and not ks.data and (ks.ld, ks.nrows, ks.ncols) == (0, n, 0)
    assert np.array_equal(A.to_words(), g.o_echelonize(a0, m, n)[0])
    assert run_dev(a0, m, n, None) is None
    H = pkg.BinMatrix.from_words(a0, n)
    assert not L.mzd_kernel_left_pluq(H.mzd, 0)
    assert np.array_equal(H.to_words(), g.o_echelonize(a0, m, n)[0])
    assert H.kernel() is None


def test_strided_view_of_a_dirty_buffer(pkg):
    """A as an offset, strided view of one buffer full of random bits: nothing outside the view changes"""
    import torch
    from m4ri_rust_amd import device
    m, n, ld, r0, cw0, nrows = 200, 321, 40, 3, 2, 210
    a0, want = R.with_pivots(m, n, list(range(0, 100)) + list(range(130, 321, 3)), seed=5)
    host = g.splitmix64(77, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld)
    aw = g.width(n)
    host[r0:r0 + m, cw0:cw0 + aw] = a0  # the excess bits of the view's last word are zero, as a gf2_dmat promises
    buf = torch.from_numpy(host.view(np.int64).copy()).cuda()
    A = device.DMat.wrap(buf.data_ptr() + 8 * (r0 * ld + cw0), m, n, ld, keep=buf)
    K, rank, piv = device.nullspace(A)
    torch.cuda.synchronize()
    after = buf.cpu().numpy().view(np.uint64)
    got_a = np.ascontiguousarray(after[r0:r0 + m, cw0:cw0 + aw])
    expect = host.copy()
    expect[r0:r0 + m, cw0:cw0 + aw] = got_a
    assert np.array_equal(after, expect), "the buffer changed outside A's view"
    six_checks(a0, m, n, K.to_words(), rank, piv, got_a, want)


@pytest.mark.parametrize("m,n,S", [(140, 130, range(65)), (320, 300, range(1, 300, 2))], ids=["single_workgroup", "blocked"])
def test_behind_pending_work_on_a_caller_stream(pkg, m, n, S):
    """A is written by a copy that waits behind a sleep on the caller's stream: the result is the serial one"""
    from m4ri_rust_amd import device
    a0, want = R.with_pivots(m, n, S, seed=m)
    aw = g.width(n)

    def call(t, s):
        K, rank, piv = device.nullspace(device.DMat.from_torch(t[0], n), stream=s)
        return K.to_words(stream=s), rank, piv

    (k, rank, piv), (got,) = on_stream(device, [padded(a0)], call)
    six_checks(a0, m, n, k, rank, piv, np.ascontiguousarray(got[:, :aw]), want)


def dirty_parent(pkg, nrows, ncols, seed):
    P = pkg.BinMatrix.zero(nrows, ncols)
    w = g.width(ncols)
    P._words_view()[:, :w] = g.splitmix64(seed, np.arange(nrows * w, dtype=np.uint64)).reshape(nrows, w)
    return P


@pytest.mark.parametrize("m,n,S", [(40, 130, range(0, 130, 5)), (320, 300, range(1, 300, 2)), (700, 900, range(100, 700))])
def test_host_entry(pkg, mode, m, n, S):
    """mzd_kernel_left_pluq on a plain matrix and on a window of a dirty parent, in both modes of the size dispatch; the host routine
    runs only below the limit of mzd_echelonize (rows * width * min(rows, cols) <= 2^20) and only in dispatch mode, and gives the
    bits of the device path"""
    L = pkg._lib.lib()
    a0, want = R.with_pivots(m, n, S, seed=m + n)
    small = mode == "dispatch" and m * g.width(n) * min(m, n) <= 1 << 20
    red, rank, piv = g.o_echelonize(a0, m, n)
    dev_k = run_dev(a0, m, n, want).to_words()
    calls = L.gf2_host_small_calls()
    H = pkg.BinMatrix.from_words(a0, n)
    K = pkg.BinMatrix(L.mzd_kernel_left_pluq(H.mzd, 0))
    six_checks(a0, m, n, K.to_words(), rank, piv, H.to_words(), want)
    assert np.array_equal(K.to_words(), dev_k), "host entry and device path differ"
    # the window at (3, 64) of a dirty parent
    r0, c0 = 3, 64
    P = dirty_parent(pkg, r0 + m + 2, c0 + n + 70, m * n)
    w = g.width(P.ncols())
    before = g.words_to_bits(P.to_words(), w * 64)
    before[r0:r0 + m, c0:c0 + n] = g.words_to_bits(a0, n)
    P._words_view()[:, :w] = g.bits_to_words(before)
    W = L.mzd_init_window(P.mzd, r0, c0, r0 + m, c0 + n)
    KW = pkg.BinMatrix(L.mzd_kernel_left_pluq(W, 0))
    L.mzd_free(W)
    expect = before.copy()
    expect[r0:r0 + m, c0:c0 + n] = g.words_to_bits(red, n)
    assert np.array_equal(g.words_to_bits(P.to_words(), w * 64), expect), "the window's reduced form, or the parent outside it"
    assert np.array_equal(KW.to_words(), want)
    assert L.gf2_host_small_calls() - calls == (2 if small else 0)


def test_kernel_methods_leave_their_receiver_unchanged(pkg, mode):
    from m4ri_rust_amd import device
    m, n, S = 320, 300, range(1, 300, 2)
    a0, want = R.with_pivots(m, n, S, seed=1)
    H = pkg.BinMatrix.from_words(a0, n)
    K = H.kernel()
    assert np.array_equal(H.to_words(), a0) and np.array_equal(K.to_words(), want)
    assert pkg._lib.lib().mzd_is_zero((H * K).mzd)
    D = device.DMat.from_words(a0, n)
    DK = D.kernel()
    assert np.array_equal(D.to_words(), a0) and np.array_equal(DK.to_words(), want)
    full = device.DMat.from_words(g.random_words(200, 130, 9), 130)
    assert full.kernel() is None


def test_bad_arguments(pkg):
    from m4ri_rust_amd import device
    L = pkg._lib.lib()
    A = device.DMat(4, 5)
    ks = pkg._lib.DMatStruct()
    rank = ctypes.c_int(0)
    assert L.gf2_nullspace_dev(None, ctypes.byref(ks), ctypes.byref(rank), None, None) == -1 and b"null" in L.gf2_last_error()
    assert L.gf2_nullspace_dev(ctypes.byref(A.s), None, ctypes.byref(rank), None, None) == -1
    assert L.gf2_nullspace_dev(ctypes.byref(A.s), ctypes.byref(ks), None, None, None) == -1
    narrow = pkg._lib.DMatStruct(A.s.data, 1, 4, 130)
    assert L.gf2_nullspace_dev(ctypes.byref(narrow), ctypes.byref(ks), ctypes.byref(rank), None, None) == -1
    assert b"stride" in L.gf2_last_error()
    empty = pkg._lib.DMatStruct(None, 0, 3, 0)
    assert L.gf2_nullspace_dev(ctypes.byref(empty), ctypes.byref(ks), ctypes.byref(rank), None, None) == 0
    assert not ks.data and ks.ncols == 0 and rank.value == 0


def test_matrix_without_rows(pkg):
    """m = 0: rank 0 and the n x n identity, also for a caller-built {NULL, 0, 0, n}"""
    from m4ri_rust_amd import device
    L = pkg._lib.lib()
    n = 70
    a = pkg._lib.DMatStruct(None, 0, 0, n)
    ks = pkg._lib.DMatStruct()
    rank = ctypes.c_int(-1)
    assert L.gf2_nullspace_dev(ctypes.byref(a), ctypes.byref(ks), ctypes.byref(rank), None, None) == 0
    assert rank.value == 0 and ks.data and (ks.nrows, ks.ncols) == (n, n)
    K = device.DMat.wrap(ks.data, n, n, ks.ld)
    K._owned = True
    assert np.array_equal(K.to_words(), g.bits_to_words(np.eye(n, dtype=np.uint8)))
