"""GPU tests of the rectangular bit-block copy (gf2_blocks.hip) and the calls built on it: gf2_copy_block_dev, gf2_submatrix_dev,
gf2_concat_dev, gf2_stack_dev through device.copy_block / submatrix / concat / stack and the DMat methods augmented, stacked,
get_window, set_window.  The reference is tests/blocks_ref.py (numpy on unpacked bits); every case compares the WHOLE destination
buffer, so the rectangle and everything outside it are checked.  The operands live in torch buffers whose row stride is the exact
width: odd strides give rows that are only 8-byte aligned, and a rectangle that ends at the last column ends at the buffer's edge."""
import ctypes

import numpy as np
import pytest

import blocks_ref as R
import gf2util as g
from stream_util import padded, run_pending

pytestmark = pytest.mark.gpu


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


def to_gpu(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def run_case(dev, c):
    s, d = R.operands(c)
    ts, td = to_gpu(s), to_gpu(d)
    dev.copy_block(dev.DMat.from_torch(td, c.d_ncols), c.dr, c.dc, dev.DMat.from_torch(ts, c.s_ncols), c.sr, c.sc, c.nrows, c.ncols,
                   accumulate=bool(c.accumulate))
    assert np.array_equal(to_host(td), R.expected(c)), c
    assert np.array_equal(to_host(ts), s), ("the source changed", c)


@pytest.mark.parametrize("src_offset", R.OFFSETS)
def test_offset_grid(dev, src_offset):
    """source offset x destination offset x width x plain / accumulate on three rows of dirty matrices"""
    mine = [c for c in R.offset_grid() if c.sc % 64 == src_offset]
    assert len(mine) == 6 * 10 * 2
    for c in mine:
        run_case(dev, c)


def test_rows(dev):
    """1, 64, 65 and 257 rows of 130 columns at offsets (5, 59): the partition of the rows among the threads"""
    for c in R.row_cases():
        run_case(dev, c)


def test_rows_at_lpn_scale(dev):
    """2^20 + 1 rows of 65 columns from offset 7 to offset 0: the grid shape at the row counts of the LPN products"""
    import torch
    nrows, ncols, sc = (1 << 20) + 1, 65, 7
    s = g.random_words(nrows, sc + ncols, 1)
    d = g.random_words(nrows, 70, 2)
    ts, td = to_gpu(s), to_gpu(d)
    dev.copy_block(dev.DMat.from_torch(td, 70), 0, 0, dev.DMat.from_torch(ts, sc + ncols), 0, sc, nrows, ncols)
    torch.cuda.synchronize()
    want = d.copy()
    with np.errstate(over="ignore"):
        want[:, 0] = (s[:, 0] >> np.uint64(7)) | (s[:, 1] << np.uint64(57))
        want[:, 1] = ((s[:, 1] >> np.uint64(7)) & np.uint64(1)) | (d[:, 1] & ~np.uint64(1))
    got = to_host(td)
    assert np.array_equal(got, want)
    # the closed form above against the reference on the first and the last rows
    head = R.copy_block(d[:70], 70, 0, 0, s[:70], sc + ncols, 0, sc, 70, ncols, False)
    tail = R.copy_block(d[-70:], 70, 0, 0, s[-70:], sc + ncols, 0, sc, 70, ncols, False)
    assert np.array_equal(want[:70], head) and np.array_equal(want[-70:], tail)


# ---- views -----------------------------------------------------------------------------------------------------------------------

def dirty(nrows, ld, seed):
    return g.splitmix64(seed, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld)


def view_of(dev, t, r0, cw0, nrows, ncols, ld):
    return dev.DMat.wrap(t.data_ptr() + 8 * (r0 * ld + cw0), nrows, ncols, ld, keep=t)


def put_view(host, r0, cw0, words):
    host[r0:r0 + words.shape[0], cw0:cw0 + words.shape[1]] = words


@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("geom", [
    # (S view: rows, cols, ld, r0, cw0, parent rows), (D view likewise), (dr, dc, sr, sc, nrows, ncols)
    ((40, 300, 9, 2, 3, 45), (50, 421, 12, 1, 2, 53), (3, 77, 5, 13, 30, 250)),
    ((40, 300, 9, 2, 3, 45), (50, 421, 12, 1, 3, 53), (0, 221, 10, 100, 30, 200)),   # ends at D's last column, 421 % 64 != 0
    ((40, 300, 10, 0, 2, 41), (50, 421, 11, 3, 1, 55), (20, 0, 0, 0, 30, 300)),      # all of S's columns, odd ld of D
], ids=["interior", "last_column", "whole_width"])
def test_strided_views_of_dirty_buffers(dev, geom, accumulate):
    """S and D are offset, strided views of buffers full of random bits: the parent of D changes in the rectangle alone (the excess
    bits of a view's last word are zero before, as a gf2_dmat promises, and after)"""
    (sm, sn, sld, sr0, scw0, sprows), (dm, dn, dld, dr0, dcw0, dprows), (dr, dc, sr, sc, nrows, ncols) = geom
    s, d = g.random_words(sm, sn, 31), g.random_words(dm, dn, 32)
    shost, dhost = dirty(sprows, sld, 33), dirty(dprows, dld, 34)
    put_view(shost, sr0, scw0, s)
    put_view(dhost, dr0, dcw0, d)
    ts, td = to_gpu(shost), to_gpu(dhost)
    dev.copy_block(view_of(dev, td, dr0, dcw0, dm, dn, dld), dr, dc, view_of(dev, ts, sr0, scw0, sm, sn, sld), sr, sc, nrows, ncols,
                   accumulate=accumulate)
    expect = dhost.copy()
    put_view(expect, dr0, dcw0, R.copy_block(d, dn, dr, dc, s, sn, sr, sc, nrows, ncols, accumulate))
    assert np.array_equal(to_host(td), expect)
    assert np.array_equal(to_host(ts), shost)


def test_rectangles_that_end_with_their_buffers(dev):
    """the source rectangle is the last bits of the last row of its buffer, and so is the destination's: the words behind them are
    not the caller's (the result is what is checked here; that they are not touched is the kernel's construction)"""
    s, d = g.random_words(4, 192, 41), g.random_words(5, 128, 42)
    ts, td = to_gpu(s), to_gpu(d)
    for acc in (False, True):
        before = to_host(td).copy()
        dev.copy_block(dev.DMat.from_torch(td, 128), 3, 36, dev.DMat.from_torch(ts, 192), 2, 100, 2, 92, accumulate=acc)
        assert np.array_equal(to_host(td), R.copy_block(before, 128, 3, 36, s, 192, 2, 100, 2, 92, acc))
    # one word to two and two to one, both at the edge
    s, d = g.random_words(2, 64, 43), g.random_words(2, 128, 44)
    ts, td = to_gpu(s), to_gpu(d)
    dev.copy_block(dev.DMat.from_torch(td, 128), 1, 33, dev.DMat.from_torch(ts, 64), 1, 0, 1, 64)
    assert np.array_equal(to_host(td), R.copy_block(d, 128, 1, 33, s, 64, 1, 0, 1, 64, False))
    d2 = g.random_words(2, 64, 45)
    td2 = to_gpu(d2)
    dev.copy_block(dev.DMat.from_torch(td2, 64), 1, 0, dev.DMat.from_torch(td, 128), 1, 33, 1, 64)
    assert np.array_equal(to_host(td2), R.copy_block(d2, 64, 1, 0, to_host(td), 128, 1, 33, 1, 64, False))


# ---- one buffer ------------------------------------------------------------------------------------------------------------------

def test_columns_of_one_matrix(dev, pkg):
    m = g.random_words(10, 300, 51)
    t = to_gpu(m)
    M = dev.DMat.from_torch(t, 300)
    dev.copy_block(M, 0, 150, M, 0, 0, 10, 100)
    want = R.copy_block(m, 300, 0, 150, m, 300, 0, 0, 10, 100, False)
    assert np.array_equal(to_host(t), want)
    # neighbours that share word 1: columns 0..99 -> 100..199
    dev.copy_block(M, 0, 100, M, 0, 0, 10, 100, accumulate=True)
    want = R.copy_block(want, 300, 0, 100, want, 300, 0, 0, 10, 100, True)
    assert np.array_equal(to_host(t), want)
    # overlapping: refused, nothing written
    L = pkg._lib.lib()
    assert L.gf2_copy_block_dev(ctypes.byref(M.s), 0, 50, ctypes.byref(M.s), 0, 0, 10, 100, 0, None) == -1
    assert b"overlap" in L.gf2_last_error()
    with pytest.raises(pkg._lib.HipError):
        dev.copy_block(M, 0, 50, M, 0, 0, 10, 100)
    assert np.array_equal(to_host(t), want)


# ---- wrappers --------------------------------------------------------------------------------------------------------------------

def no_excess(words, ncols):
    return ncols % 64 == 0 or not (words[:, -1] >> np.uint64(ncols % 64)).any()


def junk(dev, nrows, ncols, seed):
    """a destination that holds random bits in every word, the excess bits included (as a recycled block may)"""
    t = to_gpu(dirty(nrows, g.width(ncols), seed))
    return t, dev.DMat.from_torch(t, ncols)


def test_concat_stack_submatrix(dev):
    for (ar, ac), (br, bc) in R.CONCATS:
        a, b = g.random_words(ar, ac, 61), g.random_words(br, bc, 62)
        A, B = dev.DMat.from_words(a, ac), dev.DMat.from_words(b, bc)
        want = R.concat(a, ac, b, bc)
        got = dev.concat(A, B).to_words()
        assert np.array_equal(got, want) and no_excess(got, ac + bc)
        t, C = junk(dev, ar, ac + bc, 63)
        assert dev.concat(A, B, C=C) is C
        assert np.array_equal(to_host(t), want), "into a dirty destination: the excess bits come out zero"
    for (ar, ac), (br, bc) in R.STACKS:
        a, b = g.random_words(ar, ac, 64), g.random_words(br, bc, 65)
        A, B = dev.DMat.from_words(a, ac), dev.DMat.from_words(b, bc)
        want = R.stack(a, b, ac)
        assert np.array_equal(dev.stack(A, B).to_words(), want)
        t, C = junk(dev, ar + br, ac, 66)
        dev.stack(A, B, C=C)
        assert np.array_equal(to_host(t), want)
    s = g.random_words(65, 130, 67)
    S = dev.DMat.from_words(s, 130)
    want = R.submatrix(s, 130, 1, 1, 64, 129)
    assert np.array_equal(dev.submatrix(S, 1, 1, 64, 129).to_words(), want)
    t, D = junk(dev, 63, 128, 68)
    dev.submatrix(S, 1, 1, 64, 129, D=D)
    assert np.array_equal(to_host(t), want)
    t, D = junk(dev, 65, 100, 69)
    dev.submatrix(S, 0, 30, 65, 130, D=D)
    assert np.array_equal(to_host(t), R.submatrix(s, 130, 0, 30, 65, 130))
    assert np.array_equal(S.to_words(), s)


def test_concat_into_a_view_keeps_the_neighbours(dev):
    a, b = g.random_words(70, 100, 71), g.random_words(70, 29, 72)
    ld, r0, cw0 = 8, 2, 4
    host = dirty(75, ld, 73)
    t = to_gpu(host)
    dev.concat(dev.DMat.from_words(a, 100), dev.DMat.from_words(b, 29), C=view_of(dev, t, r0, cw0, 70, 129, ld))
    expect = host.copy()
    put_view(expect, r0, cw0, R.concat(a, 100, b, 29))
    assert np.array_equal(to_host(t), expect)


def test_dmat_methods_mirror_binmatrix(dev, pkg):
    a, b, c = g.random_words(70, 100, 81), g.random_words(70, 29, 82), g.random_words(3, 100, 83)
    HA, HB, HC = (pkg.BinMatrix.from_words(x, n) for x, n in ((a, 100), (b, 29), (c, 100)))
    DA, DB, DC = (dev.DMat.from_words(x, n) for x, n in ((a, 100), (b, 29), (c, 100)))
    assert np.array_equal(DA.augmented(DB).to_words(), HA.augmented(HB).to_words())
    assert np.array_equal(DA.stacked(DC).to_words(), HA.stacked(HC).to_words())
    assert np.array_equal(DA.get_window(5, 33, 69, 99).to_words(), HA.get_window(5, 33, 69, 99).to_words())
    DA.set_window(0, 70, DB)
    HA.set_window(0, 70, HB)  # bit loops on the host: 70 x 29 bits
    DA.set_window(66, 0, DC)
    HA.set_window(66, 0, HC)
    assert np.array_equal(DA.to_words(), HA.to_words())
    assert np.array_equal(DB.to_words(), b) and np.array_equal(DC.to_words(), c)


def test_get_window_then_set_window_is_the_identity(dev):
    host = dirty(40, 7, 91)
    host[:, -1] &= np.uint64((1 << 30) - 1)  # a 414-column matrix: the excess bits of its last word are zero
    t = to_gpu(host)
    P = dev.DMat.from_torch(t, 414)
    W = P.get_window(3, 61, 38, 414)
    assert np.array_equal(W.to_words(), R.submatrix(host, 414, 3, 61, 38, 414))
    P.set_window(3, 61, W)
    assert np.array_equal(to_host(t), host)


# ---- stream order ----------------------------------------------------------------------------------------------------------------

def test_copy_block_behind_a_pending_product(dev):
    """a product into C and a block update of a region of C, both on a caller's stream behind pending work: the update sees the
    product's result (the pattern of test_gpu_stream_order.py::test_add_and_transpose_dev)"""
    from test_gpu_stream_order import cut, product
    m, l, n = 300, 200, 700
    a, b, c0, ref = product(m, l, n, 17)
    s = g.random_words(120, 400, 18)
    srcs = [padded(a), padded(b), padded(c0), padded(s)]
    want = R.copy_block(ref, n, 100, 133, s, 400, 7, 29, 110, 333, True)
    want = R.copy_block(want, n, 0, 640, want, n, 200, 3, 100, 60, False)  # ... and a move inside C behind the update

    def issue(ls):
        t, st = ls[0].live, ls[0].handle
        C = dev.mul(dev.DMat.from_torch(t[0], l), dev.DMat.from_torch(t[1], n), C=dev.DMat.from_torch(t[2], n), algo="m4rm", stream=st)
        dev.copy_block(C, 100, 133, dev.DMat.from_torch(t[3], 400), 7, 29, 110, 333, accumulate=True, stream=st)
        dev.copy_block(C, 0, 640, C, 200, 3, 100, 60, stream=st)

    def check(_, outs):
        assert np.array_equal(cut(outs[0][2], n), want)
        assert np.array_equal(outs[0][3], srcs[3])

    run_pending([srcs], issue, check)
