"""GPU tests of the triangular solves (gf2_trsm.hip): gf2_trsm_dev through device.trsm and the host entries mzd_trsm_* in both
modes of the size dispatch, bit for bit against the numpy substitution, the product identity and the closed forms of
tests/trsm_ref.py; T with anything in its other triangle, the matrix mzd_pluq leaves as L and as U; strided views of one dirty
device buffer; the other block sizes the inversion kernel supports (M4RI_HIP_TRSM_BLOCK)."""
import ctypes

import numpy as np
import pytest

import gf2util as g
import trsm_ref as R

pytestmark = pytest.mark.gpu

D = 512  # TRSM_BLOCK of gf2_trsm.hip


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


def run_dev(tw, bw, n, rows, cols, upper, right):
    from m4ri_rust_amd import device
    T, B = device.DMat.from_words(tw, n), device.DMat.from_words(bw, cols)
    assert device.trsm(T, B, upper=upper, right=right) is B
    assert np.array_equal(T.to_words(), tw), "T changed"
    return B.to_words()


# a lone ragged block, an exact block, a split with a ragged tail, two levels of recursion
SIZES = [1, 63, 64, 65, 127, 129, D - 1, D, D + 1, 2 * D + 65, 1000, 4 * D + 64]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upper,right", R.VARIANTS)
def test_device_entry(pkg, n, upper, right):
    for k in (1, 65, 300) + ((4160,) if right else ()):
        R.check_variant(run_dev, n, k, upper, right, seed=31 * n + k, substitution=n <= 1000)


@pytest.mark.parametrize("d", [64, 128, 256])
def test_other_block_sizes(pkg, monkeypatch, d):
    """block sizes below the default: fewer doubling levels in the inversion kernel, more blocks in the recursion"""
    monkeypatch.setenv("M4RI_HIP_TRSM_BLOCK", str(d))
    for n in (d - 1, d + 1, 2 * d + 65):
        for upper, right in R.VARIANTS:
            R.check_variant(run_dev, n, 65, upper, right, seed=n + d)


@pytest.mark.parametrize("n", [65, 257, D + 1, 2 * D + 65])
def test_dirty_t(pkg, n):
    k = 130
    for upper, right in R.VARIANTS:
        rows, cols = R.b_shape(n, k, right)
        tb = R.random_bits(n, n, 5 * n)
        b0 = g.random_words(rows, cols, 5 * n + 1)
        want = R.solve(tb, b0, rows, cols, upper, right)
        assert np.array_equal(run_dev(g.bits_to_words(R.clean(tb, upper)), b0.copy(), n, rows, cols, upper, right), want)
        for zero_diagonal in (False, True):
            td = g.bits_to_words(R.dirty(tb, upper, 7 * n, zero_diagonal))
            assert np.array_equal(run_dev(td, b0.copy(), n, rows, cols, upper, right), want), R.name(upper, right)


def test_pluq_factors_as_l_and_u(pkg):
    """windows of what device.ple(pluq=True) leaves serve as L and as U: with the permutations, pluq_solve_left bit for bit"""
    from m4ri_rust_amd import device
    m, n, k = 300, 340, 70
    core = g.o_mul_fast(g.bits_to_words(R.clean(R.random_bits(m, m, 1), False)),
                        g.bits_to_words(R.clean(R.random_bits(m, m, 2), True)), m, m, m)  # L U: full rank
    a = g.bits_to_words(np.hstack([R.random_bits(m, n - m, 3), g.words_to_bits(core, m)]))
    A = device.DMat.from_words(a, n)
    rank, P, Q = device.ple(A, pluq=True)
    assert rank == m
    b = np.vstack([g.random_words(m, k, 4), np.zeros((n - m, g.width(k)), dtype=np.uint64)])
    want = device.DMat.from_words(b, k)
    assert device.pluq_solve_left(A, rank, P, Q, want, check=True)
    B = device.DMat.from_words(b, k)
    top = device.DMat.wrap(B.s.data, rank, k, B.ld, keep=B)           # the first r rows of B
    LU = device.DMat.wrap(A.s.data, rank, rank, A.ld, keep=A)         # the first r rows and columns of A
    device.apply_p(top, P)
    device.trsm(LU, top, upper=False)
    device.trsm(LU, top, upper=True)
    device.apply_p(B, Q, trans=True)
    assert np.array_equal(B.to_words(), want.to_words())
    assert np.array_equal(g.o_mul_fast(a, B.to_words(), m, n, k), b[:m])


@pytest.mark.parametrize("upper,right", R.VARIANTS)
def test_views_of_one_dirty_buffer(pkg, upper, right):
    """T and B as offset, strided views of one buffer full of random bits: nothing outside B's view changes, and the excess bits
    of B's last word (zero before the call, as a gf2_dmat promises) are zero afterwards"""
    import torch
    from m4ri_rust_amd import device
    n, k, ld = 321, 200, 40
    rows, cols = R.b_shape(n, k, right)
    tr, tcw, br, bcw = 3, 2, (3 if not right else 330), (10 if not right else 4)
    nrows = 540
    host = g.splitmix64(77 + 2 * upper + right, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld)
    bw = g.width(cols)
    if cols % 64:
        host[br:br + rows, bcw + bw - 1] &= np.uint64((1 << (cols % 64)) - 1)
    buf = torch.from_numpy(host.view(np.int64).copy()).cuda()
    base = buf.data_ptr()
    T = device.DMat.wrap(base + 8 * (tr * ld + tcw), n, n, ld, keep=buf)
    B = device.DMat.wrap(base + 8 * (br * ld + bcw), rows, cols, ld, keep=buf)
    device.trsm(T, B, upper=upper, right=right)
    torch.cuda.synchronize()
    after = buf.cpu().numpy().view(np.uint64)
    tb = g.words_to_bits(np.ascontiguousarray(host[tr:tr + n, tcw:tcw + g.width(n)]), n)
    b0 = np.ascontiguousarray(host[br:br + rows, bcw:bcw + bw])
    x = np.ascontiguousarray(after[br:br + rows, bcw:bcw + bw])
    assert R.no_excess(x, cols)
    expect = host.copy()
    expect[br:br + rows, bcw:bcw + bw] = x
    assert np.array_equal(after, expect), "the buffer changed outside B's view"
    assert np.array_equal(x, R.solve(tb, b0, rows, cols, upper, right))
    R.check_product(tb, x, b0, rows, cols, upper, right)


def dirty_parent(pkg, nrows, ncols, seed):
    P = pkg.BinMatrix.from_words(g.random_words(nrows, ncols, seed), ncols)
    w = g.width(ncols)
    P._words_view()[:, :w] = g.splitmix64(seed ^ 0x5EED, np.arange(nrows * w, dtype=np.uint64)).reshape(nrows, w)
    return P


def raw_bits(P):
    return g.words_to_bits(P.to_words(), g.width(P.ncols()) * 64)


HOST_ENTRY = {(False, False): "mzd_trsm_lower_left", (True, False): "mzd_trsm_upper_left",
              (False, True): "mzd_trsm_lower_right", (True, True): "mzd_trsm_upper_right"}


@pytest.mark.parametrize("n,k", [(65, 70), (300, 200), (1000, 300)])
def test_host_entries(pkg, mode, n, k):
    """plain matrices and windows of dirty parents (T and B in one parent), equal to the device result; the host routine runs
    only below the dispatch limit (n * n * ceil(k / 64) <= 2^20) and only in dispatch mode"""
    L = pkg._lib.lib()
    small = mode == "dispatch" and n * n * g.width(k) <= 1 << 20
    for upper, right in R.VARIANTS:
        fn = getattr(L, HOST_ENTRY[(upper, right)])
        rows, cols = R.b_shape(n, k, right)
        tw = g.random_words(n, n, n + k)
        b0 = g.random_words(rows, cols, n + k + 1)
        want = run_dev(tw, b0.copy(), n, rows, cols, upper, right)
        calls = L.gf2_host_small_calls()
        T, B = pkg.BinMatrix.from_words(tw, n), pkg.BinMatrix.from_words(b0, cols)
        fn(T.mzd, B.mzd, 0)
        assert np.array_equal(B.to_words(), want) and np.array_equal(T.to_words(), tw), fn.__name__
        # windows: T at (3, 64), B right of it in the same dirty parent
        bc = 64 + 64 * g.width(n) + 64
        Pm = dirty_parent(pkg, 3 + max(n, rows) + 2, bc + cols + 70, n * k)
        before = raw_bits(Pm)
        tb = before[3:3 + n, 64:64 + n]
        bwin = g.bits_to_words(before[3:3 + rows, bc:bc + cols].copy())
        TW = L.mzd_init_window(Pm.mzd, 3, 64, 3 + n, 64 + n)
        BW = L.mzd_init_window(Pm.mzd, 3, bc, 3 + rows, bc + cols)
        fn(TW, BW, 0)
        L.mzd_free(TW)
        L.mzd_free(BW)
        after = raw_bits(Pm)
        expect = before.copy()
        expect[3:3 + rows, bc:bc + cols] = g.words_to_bits(
            run_dev(g.bits_to_words(tb.copy()), bwin.copy(), n, rows, cols, upper, right), cols)
        assert np.array_equal(after, expect), fn.__name__ + ": window result or the parent outside it"
        assert L.gf2_host_small_calls() - calls == (2 if small else 0)


def test_errors(pkg):
    from m4ri_rust_amd import device
    L = pkg._lib.lib()

    def rc(T, B, right):
        return L.gf2_trsm_dev(ctypes.byref(T.s), ctypes.byref(B.s), 0, right, None)

    T, B = device.DMat(4, 5), device.DMat(4, 3)
    assert rc(T, B, 0) == -1 and b"square" in L.gf2_last_error()
    T = device.DMat(4, 4)
    assert rc(T, B, 1) == -1 and b"mismatch" in L.gf2_last_error()
    assert rc(T, device.DMat(5, 3), 0) == -1 and b"mismatch" in L.gf2_last_error()
    assert rc(device.DMat(0, 0), device.DMat(0, 5), 0) == 0
    assert rc(T, device.DMat(4, 0), 0) == 0
