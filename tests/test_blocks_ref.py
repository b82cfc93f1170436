"""Host-side tests of the device block calls, no device needed: the numpy reference tests/blocks_ref.py against the host library's
mzd_submatrix / mzd_concat / mzd_stack and against plain bit loops, and the argument checks of gf2_copy_block_dev, gf2_submatrix_dev,
gf2_concat_dev, gf2_stack_dev and gf2_solve_left_dev, which run before the first HIP call."""
import ctypes

import numpy as np
import pytest

import blocks_ref as R
import gf2util as g


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    return p


def test_reference_against_host_library_on_aligned_cases(pkg):
    """the word-aligned cases of the shared list: the rectangle of the expected D is mzd_submatrix of S (XOR that of D when
    accumulating), and nothing else of D changed"""
    aligned = [c for c in R.cases() if c.sc % 64 == 0 and c.dc % 64 == 0]
    assert len(aligned) >= 20 and any(c.accumulate for c in aligned)
    for c in aligned:
        s, d = R.operands(c)
        want = R.expected(c)
        S, D = pkg.BinMatrix.from_words(s, c.s_ncols), pkg.BinMatrix.from_words(d, c.d_ncols)
        block = S.get_window(c.sr, c.sc, c.sr + c.nrows, c.sc + c.ncols).to_words()
        if c.accumulate:
            block = block ^ D.get_window(c.dr, c.dc, c.dr + c.nrows, c.dc + c.ncols).to_words()
        W = pkg.BinMatrix.from_words(want, c.d_ncols)
        assert np.array_equal(W.get_window(c.dr, c.dc, c.dr + c.nrows, c.dc + c.ncols).to_words(), block), c
        assert np.array_equal(R.submatrix(want, c.d_ncols, c.dr, c.dc, c.dr + c.nrows, c.dc + c.ncols), block), c
        outside = g.words_to_bits(want ^ d, c.d_ncols).copy()
        outside[c.dr:c.dr + c.nrows, c.dc:c.dc + c.ncols] = 0
        assert not outside.any(), c


def test_reference_wrappers_against_host_library(pkg):
    for (ar, ac), (br, bc) in R.CONCATS:
        a, b = g.random_words(ar, ac, 1), g.random_words(br, bc, 2)
        host = pkg.BinMatrix.from_words(a, ac).augmented(pkg.BinMatrix.from_words(b, bc)).to_words()
        assert np.array_equal(R.concat(a, ac, b, bc), host)
    for (ar, ac), (br, bc) in R.STACKS:
        a, b = g.random_words(ar, ac, 3), g.random_words(br, bc, 4)
        host = pkg.BinMatrix.from_words(a, ac).stacked(pkg.BinMatrix.from_words(b, bc)).to_words()
        assert np.array_equal(R.stack(a, b, ac), host)
    s = g.random_words(65, 130, 5)
    assert np.array_equal(R.submatrix(s, 130, 1, 1, 64, 129), pkg.BinMatrix.from_words(s, 130).get_window(1, 1, 64, 129).to_words())


def bit(words, r, c):
    return (int(words[r, c // 64]) >> (c % 64)) & 1


@pytest.mark.parametrize("c", [R.Case(3, 70, 1, 61, 2, 9, 0, 3, 2, 6, 0, 11), R.Case(2, 130, 0, 63, 3, 131, 1, 1, 2, 67, 1, 12),
                               R.Case(1, 5, 0, 2, 1, 66, 0, 62, 1, 3, 0, 13)], ids=["into_two_words", "accumulate", "from_two_words"])
def test_reference_against_bit_loops(c):
    s, d = R.operands(c)
    want = R.expected(c)
    for r in range(c.d_rows):
        for col in range(g.width(c.d_ncols) * 64):
            i, j = r - c.dr, col - c.dc
            old = bit(d, r, col)
            if 0 <= i < c.nrows and 0 <= j < c.ncols:
                src = bit(s, c.sr + i, c.sc + j)
                assert bit(want, r, col) == (old ^ src if c.accumulate else src), (r, col)
            else:
                assert bit(want, r, col) == old, (r, col)


def test_shared_list_has_every_offset_pair():
    grid = R.offset_grid()
    assert len(grid) == 6 * 6 * 10 * 2
    assert {(c.sc % 64, c.dc % 64) for c in grid} == {(a, b) for a in R.OFFSETS for b in R.OFFSETS}
    for a in R.OFFSETS:
        for b in R.OFFSETS:
            assert {((c.sc // 64) & 1, (c.dc // 64) & 1) for c in grid if (c.sc % 64, c.dc % 64) == (a, b)} == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- argument checks, before the first HIP call: made-up pointers are never dereferenced ------------------------------------------

def mat(pkg, addr, ld, nrows, ncols):
    return pkg._lib.DMatStruct(addr, ld, nrows, ncols)


def refused(L, rc, *names):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    for name in names:
        assert name in msg, msg


def test_bad_arguments_are_refused_without_a_device(pkg):
    L = pkg._lib.lib()
    ref = ctypes.byref
    S, D = mat(pkg, 0x10000, 4, 10, 200), mat(pkg, 0x90000, 6, 12, 300)
    cb = L.gf2_copy_block_dev
    refused(L, cb(ref(D), 0, 0, ref(S), 0, 101, 5, 100, 0, None), "gf2_copy_block_dev", "leaves S")
    refused(L, cb(ref(D), 0, 0, ref(S), 6, 0, 5, 100, 0, None), "leaves S")
    refused(L, cb(ref(D), 0, 201, ref(S), 0, 0, 5, 100, 0, None), "leaves D")
    refused(L, cb(ref(D), 8, 0, ref(S), 0, 0, 5, 100, 0, None), "leaves D")
    refused(L, cb(ref(D), 0, 0, ref(S), 0, 0, 5, -1, 0, None), "ncols")
    refused(L, cb(ref(D), 0, 0, ref(S), 0, 0, -5, 1, 0, None), "nrows")
    refused(L, cb(ref(D), 0, -1, ref(S), 0, 0, 5, 1, 0, None), "dc")
    refused(L, cb(None, 0, 0, ref(S), 0, 0, 5, 1, 0, None), "D", "null")
    refused(L, cb(ref(D), 0, 0, None, 0, 0, 5, 1, 0, None), "S", "null")
    refused(L, cb(ref(D), 0, 0, ref(mat(pkg, None, 4, 10, 200)), 0, 0, 5, 1, 0, None), "S.data")
    refused(L, cb(ref(D), 0, 0, ref(mat(pkg, 0x10000, 3, 10, 200)), 0, 0, 5, 1, 0, None), "S.ld")
    # empty rectangles: nothing to do, no launch, no device needed
    assert cb(ref(D), 0, 0, ref(S), 0, 0, 0, 100, 0, None) == 0
    assert cb(ref(D), 12, 300, ref(S), 10, 200, 0, 0, 1, None) == 0
    assert cb(ref(D), 3, 7, ref(S), 1, 1, 4, 0, 0, None) == 0

    refused(L, L.gf2_submatrix_dev(ref(mat(pkg, 0x90000, 2, 5, 99)), ref(S), 0, 0, 5, 100, None), "gf2_submatrix_dev", "D must be")
    refused(L, L.gf2_submatrix_dev(ref(mat(pkg, 0x90000, 2, 5, 100)), ref(S), 8, 0, 13, 100, None), "leaves S")
    refused(L, L.gf2_submatrix_dev(ref(mat(pkg, 0x90000, 2, 5, 100)), ref(S), 5, 0, 4, 100, None), "highr")
    assert L.gf2_submatrix_dev(ref(mat(pkg, None, 0, 0, 100)), ref(S), 5, 0, 5, 100, None) == 0

    A, B = mat(pkg, 0x10000, 2, 7, 100), mat(pkg, 0x20000, 2, 8, 29)
    refused(L, L.gf2_concat_dev(ref(mat(pkg, 0x90000, 4, 7, 129)), ref(A), ref(B), None), "gf2_concat_dev", "A.nrows", "B.nrows")
    B7 = mat(pkg, 0x20000, 2, 7, 29)
    refused(L, L.gf2_concat_dev(ref(mat(pkg, 0x90000, 4, 7, 128)), ref(A), ref(B7), None), "C must be")
    refused(L, L.gf2_concat_dev(ref(mat(pkg, 0x10000, 4, 7, 129)), ref(A), ref(B7), None), "overlap")  # C on top of A
    refused(L, L.gf2_stack_dev(ref(mat(pkg, 0x90000, 2, 15, 100)), ref(A), ref(B), None), "gf2_stack_dev", "A.ncols", "B.ncols")
    B100 = mat(pkg, 0x20000, 2, 8, 100)
    refused(L, L.gf2_stack_dev(ref(mat(pkg, 0x90000, 2, 14, 100)), ref(A), ref(B100), None), "C must be")

    bad = ctypes.c_int(7)
    refused(L, L.gf2_solve_left_dev(ref(mat(pkg, 0x10000, 4, 100, 200)), ref(mat(pkg, 0x90000, 2, 150, 70)), 1, ref(bad), None),
            "gf2_solve_left_dev", "A.ncols", "B.nrows")
    refused(L, L.gf2_solve_left_dev(ref(mat(pkg, 0x10000, 4, 200, 100)), ref(mat(pkg, 0x90000, 2, 150, 70)), 1, ref(bad), None),
            "A.nrows", "B.nrows")
    refused(L, L.gf2_solve_left_dev(None, ref(D), 1, ref(bad), None), "null")
    refused(L, L.gf2_solve_left_dev(ref(S), ref(D), 1, None, None), "null")
    for a, b in ((mat(pkg, 0x10000, 4, 0, 5), mat(pkg, 0x90000, 2, 9, 70)), (mat(pkg, 0x10000, 4, 5, 0), mat(pkg, 0x90000, 2, 9, 70)),
                 (mat(pkg, 0x10000, 4, 5, 5), mat(pkg, 0x90000, 2, 9, 0))):
        bad.value = 7
        assert L.gf2_solve_left_dev(ref(a), ref(b), 1, ref(bad), None) == 0 and bad.value == 0


def test_overlap_rule_without_a_device(pkg):
    """rectangles of one buffer: compared exactly with one ld, by address range with two"""
    L = pkg._lib.lib()
    ref = ctypes.byref
    cb = L.gf2_copy_block_dev
    base, ld = 0x40000, 6
    M = mat(pkg, base, ld, 10, 300)
    refused(L, cb(ref(M), 0, 50, ref(M), 0, 0, 10, 100, 0, None), "overlap")
    refused(L, cb(ref(M), 0, 99, ref(M), 0, 0, 10, 100, 0, None), "overlap")
    refused(L, cb(ref(M), 3, 0, ref(M), 0, 0, 4, 100, 0, None), "overlap")  # rows 0..3 onto rows 3..6
    # two views of the parent whose rectangles are the same bits: D starts one row and two words further on
    V = mat(pkg, base + 8 * (ld + 2), ld, 8, 100)
    refused(L, cb(ref(V), 0, 0, ref(M), 1, 128, 3, 50, 0, None), "overlap")
    refused(L, cb(ref(V), 0, 10, ref(M), 2, 100, 3, 50, 0, None), "overlap")  # both reach the parent's row 2 in columns 138..149
    # a view that starts left of S's first word, one row down: the same addresses once more
    W = mat(pkg, base + 8 * (ld - 1), ld, 8, 300)
    refused(L, cb(ref(W), 0, 64, ref(mat(pkg, base, ld, 10, 300)), 1, 0, 2, 10, 0, None), "overlap")
    # different ld, intersecting address ranges: refused although no bit is shared
    N = mat(pkg, base, 3, 20, 150)
    refused(L, cb(ref(N), 0, 0, ref(M), 0, 250, 2, 50, 0, None), "overlap")


def test_new_symbols_are_declared(pkg):
    for name in ("gf2_copy_block_dev", "gf2_submatrix_dev", "gf2_concat_dev", "gf2_stack_dev", "gf2_solve_left_dev"):
        assert name in pkg._lib.DECLARED_SYMBOLS and getattr(pkg._lib.lib(), name)
