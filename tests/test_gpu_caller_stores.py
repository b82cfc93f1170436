"""Stores through rows[] after a product, under the shipped defaults: m4ri-sys's mzd_write_bit, BinMatrix::set_window and
get_word_mut write the host words directly, so the library never sees them.  Whatever it keeps beside a product (the result side
copy of a thin product, m4ri_hip_api.cpp ResultSide) must not outlive such a store: the next mzd_transpose -- and the reference's
`mul_slice` -> store -> `as_vector` chain, which is one -- has to return the stored bits.  No knob, no gf2_mzd_uncache here."""
import numpy as np
import pytest

import gf2util as g

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


def _store(view, ref, m, n):
    """one store in the first row (a single bit), a middle row (a whole word, inside the row) and the last row (a single bit)"""
    full = np.uint64((1 << n) - 1) if n < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    st = ref.copy()
    for row, word in ((0, np.uint64(1)), (m // 2, full), (m - 1, np.uint64(1 << (n - 1)))):
        view[row, 0] ^= word
        st[row, 0] ^= word
    return st


@pytest.mark.parametrize("m,n", [(1 << 20, 1), (1 << 18, 3), (300001, 2), (1 << 17, 8)])
@pytest.mark.parametrize("cached", [False, True])
def test_store_after_a_product_is_seen_by_transpose(pkg, m, n, cached):
    L = pkg._lib.lib()
    l = 256
    a, x = g.random_words(m, l, 3), g.random_words(l, n, 4)
    A, X = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(x, n)
    if cached:
        A.cache_on_device()
    ref = g.o_mul_naive(a, x, m, l, n)
    R = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))  # a fresh product into NULL
    assert np.array_equal(R.to_words(), ref)
    st = _store(R._words_view(), ref, m, n)
    want = g.o_transpose(st, m, n)
    T = pkg.BinMatrix(L.mzd_transpose(None, R.mzd))
    assert np.array_equal(T.to_words(), want), "mzd_transpose(NULL, R) returned the bits from before the store"
    T2 = pkg.BinMatrix.zero(n, m)
    assert L.mzd_transpose(T2.mzd, R.mzd) and np.array_equal(T2.to_words(), want), "mzd_transpose(T, R) returned stale bits"
    if cached:
        A.uncache()


@pytest.mark.parametrize("cached", [False, True])
def test_mul_slice_store_as_vector(pkg, cached):
    """binary_matrix.rs: `let mut y = a.mul_slice(v); <store into y>; y.as_vector()` with a raw store (not the friendly set_window,
    which tells the library)."""
    m, l = 1 << 20, 256
    a = g.random_words(m, l, 5)
    A = pkg.BinMatrix.from_words(a, l)
    if cached:
        A.cache_on_device()
    v = g.random_words(1, l, 6)[0]
    y = A.mul_slice(v)
    ref = g.o_mul_naive(a, g.o_transpose(v.reshape(1, -1), 1, l), m, l, 1)
    assert np.array_equal(y.to_words(), ref)
    st = _store(y._words_view(), ref, m, 1)
    got = y.as_vector()
    assert len(got) == m and np.array_equal(np.asarray(got.get_storage(), dtype=np.uint64), g.o_transpose(st, m, 1)[0])
    if cached:
        A.uncache()
