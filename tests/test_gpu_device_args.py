"""GPU tests of the Python wrappers of m4ri_rust_amd/device.py themselves, not of the kernels behind them: the ValueErrors the wrappers
raise before (or between) their C calls, and what comes back for an output array that is None, a raw device address or SKIP.

The pools are tiny -- 8 rows of 70 columns: two words, the last one ragged, b = 2 -- except where a count has to pass 2^31: there no
row is stored and only the count kernels run.  Every address handed to an entry comes from a live torch tensor or DMat."""
import numpy as np
import pytest

import gf2util as g
import join_ref as jr

pytestmark = pytest.mark.gpu

N, NCOLS, B = 8, 70, 2


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


@pytest.fixture(scope="module")
def pool(dev):
    """(words, DMat) of the 8 x 70 pool"""
    wa = g.random_words(N, NCOLS, 11)
    return wa, dev.DMat.from_words(wa, NCOLS)


@pytest.fixture(scope="module")
def big(dev):
    """46341 x 64: 46341^2 = 2 147 488 281 ordered pairs, the first square past 2^31"""
    return dev.DMat.random(46341, 64, 5)


def ints(n, dtype="int32", fill=-7):
    import torch
    return torch.full((max(n, 1),), fill, dtype=getattr(torch, dtype), device="cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def is_owned(x, count=None):
    """an array the wrapper allocated: an address, the count, the matrix behind it and a read() that waits"""
    if x is None or not isinstance(x.ptr, int) or x.ptr == 0 or x.mat is None or not hasattr(x, "read"):
        return False
    return count is None or x.count == count


# ---- ValueErrors ----------------------------------------------------------------------------------------------------------------------

def test_a_raw_count_address_needs_D_or_cap(dev, pool):
    A = pool[1]
    c32, c64 = ints(2), ints(2, "int64")
    calls = {
        "lf1_reduce": lambda: dev.lf1_reduce(A, 0, B, count=c32.data_ptr()),
        "lf2_reduce": lambda: dev.lf2_reduce(A, 0, B, count=c64.data_ptr()),
        "join": lambda: dev.join(A, A, 0, B, count=c64.data_ptr()),
        "join_select": lambda: dev.join_select(A, A, 0, B, None, 0, NCOLS, hits=c64.data_ptr()),
        "near_pairs": lambda: dev.near_pairs(A, A, None, 0, NCOLS, hits=c64.data_ptr()),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="^%s: a raw (count|hits) address needs D or cap" % name):
            call()
    assert np.all(host(c32) == -7) and np.all(host(c64) == -7)              # refused before any call


def test_store_false_takes_no_D(dev, pool):
    A = pool[1]
    D = dev.DMat(4, NCOLS)
    with pytest.raises(ValueError, match="^join_select: store=False takes no D"):
        dev.join_select(A, A, 0, B, None, 0, NCOLS, D=D, store=False)
    with pytest.raises(ValueError, match="^near_pairs: store=False takes no D"):
        dev.near_pairs(A, A, None, 0, NCOLS, D=D, store=False)
    with pytest.raises(ValueError, match="^subset_sums: store=False takes no D"):
        dev.subset_sums(A, 2, D=D, store=False)


def test_subset_sums_arguments(dev, pool):
    A = pool[1]
    with pytest.raises(ValueError, match="^subset_sums: count = 3, but D has 4 rows"):
        dev.subset_sums(A, 2, count=3, D=dev.DMat(4, NCOLS))
    with pytest.raises(ValueError, match="^subset_sums: p = 5 is outside 1 .. 4"):
        dev.subset_sums(A, 5)


def test_gathers_check_their_indices(dev, pool):
    A = pool[1]
    idx = ints(3, fill=0)
    with pytest.raises(ValueError, match="^gather_rows: a raw idx address needs D"):
        dev.gather_rows(A, idx.data_ptr())
    with pytest.raises(ValueError, match="^gather_cols: a raw idx address needs D"):
        dev.gather_cols(A, idx.data_ptr())
    with pytest.raises(ValueError, match="^gather_rows: idx holds 3 indices, D needs 2"):
        dev.gather_rows(A, [0, 1, 2], D=dev.DMat(2, NCOLS))
    with pytest.raises(ValueError, match="^gather_cols: idx holds 3 indices, D needs 2"):
        dev.gather_cols(A, [0, 1, 2], D=dev.DMat(N, 2))
    for bad in (np.array([0.0, 1.0]), np.array([0, 1 << 31])):
        with pytest.raises(ValueError, match="^gather_rows: idx must hold int32 values"):
            dev.gather_rows(A, bad)
        with pytest.raises(ValueError, match="^gather_cols: idx must hold int32 values"):
            dev.gather_cols(A, bad)


def test_uploaded_arrays_are_checked_under_the_wrappers_name(dev):
    with pytest.raises(ValueError, match="^select_weights: idx holds 3 indices, D needs 2"):
        dev.select_weights([1, 2, 3], 2, 0, 9)
    with pytest.raises(ValueError, match="^min_weight: idx holds 3 indices, D needs 2"):
        dev.min_weight([1, 2, 3], 2)
    with pytest.raises(ValueError, match="^unrank_subsets: idx holds 3 indices, D needs 2"):
        dev.unrank_subsets([0, 1, 2], 2, 2, N)
    with pytest.raises(ValueError, match="^select_weights: idx must hold int32 values"):
        dev.select_weights([0.5, 1.5], 2, 0, 9)
    with pytest.raises(ValueError, match="^min_weight: idx must hold int32 values"):
        dev.min_weight([0, 1 << 31], 2)


# ---- counts that do not fit a matrix: the count-only call, then the refusal -------------------------------------------------------------

def test_join_pairs_do_not_fit_a_matrix(dev, big):
    with pytest.raises(ValueError, match="^join: 2147488281 pairs do not fit a matrix; give D or cap"):
        dev.join(big, big, 0, 0)


def test_lf2_pairs_do_not_fit_a_matrix(dev):
    P = dev.DMat.random(65537, 64, 6)
    with pytest.raises(ValueError, match="^lf2_reduce: 2147516416 pairs do not fit a matrix; give D or cap"):
        dev.lf2_reduce(P, 0, 0)


def test_join_select_hits_do_not_fit_a_matrix(dev, big):
    with pytest.raises(ValueError, match="^join_select: 2147488281 hits do not fit a matrix; give D or cap"):
        dev.join_select(big, big, 0, 0, None, 0, 64)


def test_near_pairs_hits_do_not_fit_a_matrix(dev, big):
    with pytest.raises(ValueError, match="^near_pairs: 2147488281 hits do not fit a matrix; give D or cap"):
        dev.near_pairs(big, big, None, 0, 64)


# ---- what comes back: None, a raw address, SKIP -------------------------------------------------------------------------------------------

def test_row_weights_waits_and_returns_numpy(dev, pool):
    wa, A = pool
    want = jr.weights(wa, 0, NCOLS)
    got = dev.row_weights(A)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want)
    t = ints(N + 1)
    assert dev.row_weights(A, out=t.data_ptr()) is None
    assert np.array_equal(host(t)[:N], want) and host(t)[N] == -7
    empty = dev.row_weights(dev.DMat.wrap(0, 0, NCOLS, 2))
    assert isinstance(empty, np.ndarray) and empty.dtype == np.int32 and len(empty) == 0


def test_join_returns_objects(dev, pool):
    wa, A = pool
    want = jr.join(wa, wa, NCOLS, 0, B)
    n = want.count
    assert 0 < n == len(want.ia)
    # None: the count-first call sizes D, every array is an object
    D, count, ia, ib, wt = dev.join(A, A, 0, B)
    assert D.nrows == n and np.array_equal(D.to_words(), want.D)
    assert is_owned(count, 2) and count.read(None).dtype == np.int64 and list(count.read(None)) == [n]
    for own, rows in ((ia, want.ia), (ib, want.ib), (wt, want.wt)):
        assert is_owned(own, n) and own.read(None).dtype == np.int32 and np.array_equal(own.read(None), rows)
    # raw addresses: None in their place, the data in the caller's tensors
    tc, ta, tb, tw = ints(1, "int64"), ints(n + 1), ints(n + 1), ints(n + 1)
    D2 = dev.DMat(n, NCOLS)
    out = dev.join(A, A, 0, B, D=D2, count=tc.data_ptr(), ia=ta.data_ptr(), ib=tb.data_ptr(), wt=tw.data_ptr())
    assert out[0] is D2 and out[1:] == (None, None, None, None)
    assert host(tc)[0] == n and np.array_equal(D2.to_words(), want.D)
    for t, rows in ((ta, want.ia), (tb, want.ib), (tw, want.wt)):
        assert np.array_equal(host(t)[:n], rows) and host(t)[n] == -7
    # SKIP: None in their place; cap: the capacity without a count-first call
    D3, count, ia, ib, wt = dev.join(A, A, 0, B, cap=n + 3, ia=dev.SKIP, ib=dev.SKIP, wt=dev.SKIP)
    assert (ia, ib, wt) == (None, None, None) and D3.nrows == n + 3 and is_owned(count, 2) and list(count.read(None)) == [n]
    assert np.array_equal(D3.to_words()[:n], want.D)


def test_nearest_always_allocates(dev, pool):
    wa, A = pool
    wb = g.random_words(5, NCOLS, 12)
    Bm = dev.DMat.from_words(wb, NCOLS)
    d = (g.words_to_bits(wa, NCOLS)[:, None, :] ^ g.words_to_bits(wb, NCOLS)[None, :, :]).sum(axis=2)
    want_i, want_d = d.argmin(axis=1), d.min(axis=1)
    idx, dist = dev.nearest(A, Bm)
    assert is_owned(idx, N) and is_owned(dist, N)
    assert idx.read(None).dtype == np.int32 and np.array_equal(idx.read(None), want_i) and np.array_equal(dist.read(None), want_d)
    ti, td = ints(N + 1), ints(N + 1)
    assert dev.nearest(A, Bm, idx=ti.data_ptr(), dist=td.data_ptr()) == (None, None)
    assert np.array_equal(host(ti)[:N], want_i) and np.array_equal(host(td)[:N], want_d) and host(ti)[N] == -7 and host(td)[N] == -7
    idx, dist = dev.nearest(A, Bm, idx=dev.SKIP)
    assert idx is None and is_owned(dist, N) and np.array_equal(dist.read(None), want_d)
    idx, dist = dev.nearest(A, Bm, dist=dev.SKIP)
    assert dist is None and is_owned(idx, N) and np.array_equal(idx.read(None), want_i)


def test_a_pool_of_no_rows(dev, pool):
    A = pool[1]
    E = dev.DMat.wrap(0, 0, NCOLS, 2)
    D, count, ia, ib, wt = dev.join(E, E, 0, B)
    assert D.nrows == 0 and D.ncols == NCOLS and (ia, ib, wt) == (None, None, None)      # nothing to allocate
    assert is_owned(count, 2) and list(count.read(None)) == [0]
    idx, dist = dev.nearest(E, A)                                                       # an address all the same
    assert is_owned(idx, 0) and is_owned(dist, 0) and len(idx.read(None)) == 0 and len(dist.read(None)) == 0
    order, skeys = dev.class_sort(E, 0, B)
    assert is_owned(order, 0) and is_owned(skeys, 0) and len(order.read(None)) == 0 and len(skeys.read(None)) == 0
    assert order.read(None).dtype == np.int32
