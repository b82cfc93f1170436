"""The aliasing contract of the device-resident API (include/m4ri_hip.h section 2) on the device: every "allowed" row of the header's
table is run with arguments that are, or overlap, one buffer, and compared bit for bit with the oracle (gf2util) or numpy XOR; every
"refused" row is made once more with live buffers.  tests/test_dev_contract.py pins the same table without a device.

The operands are views of torch buffers filled with random bits (the excess bits of each view zeroed, as a gf2_dmat promises), and every
case compares EVERY word of the parent outside the written view as well.  The module's name sorts before tests/test_zz_kernel_census.py."""
import ctypes
import functools

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
from census_util import assert_route, census
from limits_ref import sample_rows

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


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def even(w):
    return (w + 1) & ~1


class Parent:
    """nrows x ld words of random bits on the device, and what the host expects them to be"""

    def __init__(self, nrows, ld, seed):
        import torch
        self.host = g.splitmix64(seed ^ 0xA11A5, np.arange(nrows * ld, dtype=np.uint64)).reshape(nrows, ld).copy()
        self.ld, self.buf, self._torch = ld, None, torch

    def put(self, r0, w0, words):
        """the words of a matrix (zero excess bits) at row r0, word w0; before upload()"""
        assert self.buf is None and r0 + words.shape[0] <= self.host.shape[0] and w0 + words.shape[1] <= self.ld
        self.host[r0:r0 + words.shape[0], w0:w0 + words.shape[1]] = words
        return self

    def upload(self):
        self.buf = self._torch.from_numpy(self.host.view(np.int64).copy()).cuda()
        return self

    def view(self, dev, r0, w0, nrows, ncols):
        assert r0 + nrows <= self.host.shape[0] and w0 + g.width(ncols) <= self.ld
        return dev.DMat.wrap(self.buf.data_ptr() + 8 * (r0 * self.ld + w0), nrows, ncols, self.ld, keep=self.buf)

    def read(self):
        self._torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint64)

    def check(self, what, r0=0, w0=0, want=None):
        """the words `want` at (r0, w0), every other word of the parent as it was"""
        expect = self.host.copy()
        if want is not None:
            expect[r0:r0 + want.shape[0], w0:w0 + want.shape[1]] = want
        got = self.read()
        bad = np.argwhere(got != expect)
        assert not len(bad), "%s: %d wrong words in the parent, first at (row, word) %s; the written view starts at (%d, %d)" % (
            what, len(bad), tuple(bad[0]), r0, w0)


def routed(L, families, fn):
    k0 = census(L)
    out = fn()
    assert_route(k0, census(L), families)
    return out


# ---- gf2_add_dev in place ---------------------------------------------------------------------------------------------------------------

ADD_SHAPES = [(1, 1), (3, 64), (5, 65), (70, 129), (257, 1000), (1000, 4097)]
# (name, ld for a row of w words, first row, first word): a dense matrix; a view with ld = width + 2 at row 1, word 2; rows that are only
# 8-byte aligned: an odd ld, and an even ld with the base at an odd word
LAYOUTS = [("dense", lambda w: w if w == 1 else even(w), 0, 0), ("view", lambda w: w + 2, 1, 2),
           ("odd-ld", lambda w: (w + 2) | 1, 1, 2), ("odd-base", lambda w: even(w + 3), 1, 3)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=[x[0] for x in LAYOUTS])
@pytest.mark.parametrize("nrows,ncols", ADD_SHAPES)
def test_add_in_place(L, dev, nrows, ncols, layout):
    """C is A, C is B, C is A is B: what mzd_add(self, self, other) means.  The shapes: one word, one pair, a pair and the single-word
    tail (65, 129 columns: an odd word count), several blocks."""
    name, ld_of, r0, w0 = layout
    w = g.width(ncols)
    ld, rows = ld_of(w), nrows + (2 if r0 else 0)
    if name == "odd-ld":
        assert ld % 2 == 1
    if name == "odd-base":
        assert ld % 2 == 0 and w0 % 2 == 1
    a, b = g.random_words(nrows, ncols, 7 * nrows + ncols), g.random_words(nrows, ncols, 7 * nrows + ncols + 1)
    for case in ("C is A", "C is B", "C is A is B"):
        PA = Parent(rows, ld, nrows + ncols).put(r0, w0, a).upload()
        PB = Parent(rows, ld, nrows + ncols + 50).put(r0, w0, b).upload()
        A, B = PA.view(dev, r0, w0, nrows, ncols), PB.view(dev, r0, w0, nrows, ncols)
        A2 = PA.view(dev, r0, w0, nrows, ncols)  # the same view in a second struct
        if case == "C is A":
            routed(L, ["gf2_xor2d_kernel"], lambda: dev.add(A, B, C=A2))
            want = a ^ b
        elif case == "C is B":
            routed(L, ["gf2_xor2d_kernel"], lambda: dev.add(B, A, C=A2))
            want = a ^ b
        else:
            routed(L, ["gf2_xor2d_kernel"], lambda: dev.add(A, A2, C=A))
            want = np.zeros_like(a)
        PA.check("%s, %s" % (case, name), r0, w0, want)
        PB.check("%s, %s: the other operand" % (case, name))


# ---- squaring and the Gram matrix -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def square_ref(n):
    a = g.random_words(n, n, 900 + n)
    c0 = g.random_words(n, n, 901 + n)
    sq = g.o_mul_fast(a, a, n, n, n)
    for x in (a, c0, sq):
        x.setflags(write=False)
    return a, c0, sq


def result_parent(m, n, c0, seed):
    """C as an m x n view at row 1, word 2 of a dirty parent with an even stride (16-byte aligned rows: every product path applies)"""
    w = g.width(n)
    P = Parent(m + 2, even(w) + 4, seed)
    if c0 is not None:
        P.put(1, 2, c0)
    else:  # a valid gf2_dmat: zero excess bits
        P.put(1, 2, g.random_words(m, n, seed + 3))
    return P.upload()


ALGOS = [("naive", 0), ("m4rm", 0), ("strassen", 1), ("auto", 0)]


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("algo,param", ALGOS, ids=[a for a, _ in ALGOS])
@pytest.mark.parametrize("n", [300, 2048])
def test_squaring(L, dev, n, algo, param, acc):
    """gf2_mul_dev(C, A, A): both operands are one struct, and one buffer under two structs"""
    a, c0, sq = square_ref(n)
    PA = Parent(n, even(g.width(n)), n).put(0, 0, a).upload()
    for A, B in ((PA.view(dev, 0, 0, n, n),) * 2, (PA.view(dev, 0, 0, n, n), PA.view(dev, 0, 0, n, n))):
        PC = result_parent(n, n, c0 if acc else None, 40 + n)
        C = PC.view(dev, 1, 2, n, n)
        k0 = census(L)
        dev.mul(A, B, C, accumulate=bool(acc), algo=algo, param=param)
        PC.check("A * A, %s" % algo, 1, 2, sq ^ c0 if acc else sq)
        PA.check("the operand of A * A")
        if algo == "strassen" and n == 2048:
            assert_route(k0, census(L), ["gf2_strassen_"])
        if algo == "m4rm":
            assert_route(k0, census(L), ["gf2_m4rm_kernel"])


def test_the_planner_squares_2048_with_one_strassen_level(L, dev):
    kind, dims = ctypes.c_int(), (ctypes.c_int * 3)()
    for n in (2048, 4096):
        assert L.gf2_mul_plan(n, n, n, dev.ALGOS["strassen"], 1, ctypes.byref(kind), dims) == 1 and kind.value == 0


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("algo,param", ALGOS, ids=[a for a, _ in ALGOS])
def test_squaring_4096_against_a_separate_copy(L, dev, algo, param, acc):
    """what sharing the buffer changes, without a second oracle product: A * A with B the same buffer against A * A' with A' a copy of
    A's bits elsewhere"""
    n = 4096
    A = dev.DMat.random(n, n, 77)
    Acopy = dev.DMat.random(n, n, 77)
    shared, apart = dev.DMat.random(n, n, 78), dev.DMat.random(n, n, 78)
    dev.mul(A, A, shared, accumulate=bool(acc), algo=algo, param=param)
    dev.mul(A, Acopy, apart, accumulate=bool(acc), algo=algo, param=param)
    assert dev.equal(shared, apart)
    assert dev.equal(A, Acopy), "an operand changed"
    assert not dev.equal(shared, dev.DMat.random(n, n, 78)), "the product left C as it was"


# 200 x 300: the row-parity kernel.  32 x 9000: a wave per row (at most 32 vectors of 8192 bits or more); 40 x 9000 has 40 vectors and
# stays with the row-parity kernel under the shipped thresholds -- the census says which one ran.
GRAM = [(200, 300, "gf2_rowparity_kernel"), (40, 9000, "gf2_rowparity_kernel"), (32, 9000, "gf2_widevec_kernel")]


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("m,l,family", GRAM, ids=["%dx%d" % (m, l) for m, l, _ in GRAM])
def test_gram_matrix(L, dev, m, l, family, acc):
    """gf2_mul_nt_dev(C, A, A) = A A^T: symmetric, and the oracle's"""
    a = g.random_words(m, l, 500 + m)
    c0 = g.random_words(m, m, 501 + m)
    gram = g.o_mul_fast(a, g.o_transpose(a, m, l), m, l, m)
    bits = g.words_to_bits(gram, m)
    assert np.array_equal(bits, bits.T)
    PA = Parent(m + 2, g.width(l) + 3, m).put(1, 1, a).upload()   # an odd word offset: 8-byte aligned rows
    for A, Bt in ((PA.view(dev, 1, 1, m, l),) * 2, (PA.view(dev, 1, 1, m, l), PA.view(dev, 1, 1, m, l))):
        PC = result_parent(m, m, c0 if acc else None, 60 + m)
        C = PC.view(dev, 1, 2, m, m)
        routed(L, [family], lambda: dev.mul_nt(A, Bt, C, accumulate=bool(acc)))
        PC.check("A A^T", 1, 2, gram ^ c0 if acc else gram)
        if not acc:
            got = g.words_to_bits(np.ascontiguousarray(PC.read()[1:1 + m, 2:2 + g.width(m)]), m)
            assert np.array_equal(got, got.T), "A A^T is not symmetric"
        PA.check("the operand of A A^T")


def test_operands_that_overlap_read_only(L, dev):
    """A = rows 0 .. 2047 and B = rows 64 .. 2111 of one parent: 1984 rows belong to both"""
    n, ld = 2048, 32
    P = Parent(2112, ld, 5).upload()
    A, B = P.view(dev, 0, 0, n, n), P.view(dev, 64, 0, n, n)
    rows = sample_rows(n, ld, 11)
    a = np.ascontiguousarray(P.host[rows])
    b = np.ascontiguousarray(P.host[64:64 + n])
    want = g.o_mul_fast(a, b, len(rows), n, n)
    for algo, param in ALGOS:
        PC = result_parent(n, n, None, 70)
        dev.mul(A, B, PC.view(dev, 1, 2, n, n), algo=algo, param=param)
        got = PC.read()
        assert np.array_equal(got[1 + rows, 2:2 + g.width(n)], want), algo
        mask = np.ones(got.shape, dtype=bool)
        mask[1:1 + n, 2:2 + g.width(n)] = False
        assert np.array_equal(got[mask], PC.host[mask]), "the parent of C changed outside C"
        P.check("the parent of A and B")


# ---- one arena --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def arena_product(m, l, n):
    a, b, c0 = g.random_words(m, l, 300 + m), g.random_words(l, n, 301 + m), g.random_words(m, n, 302 + m)
    prod = g.o_mul_fast(a, b, m, l, n)
    for x in (a, b, c0, prod):
        x.setflags(write=False)
    return a, b, c0, prod


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("m,l,n", [(300, 200, 130), (2048, 2048, 2048)])
def test_product_in_one_arena(L, dev, m, l, n, acc):
    """C, A and B are three disjoint column ranges of one dirty parent with one ld"""
    a, b, c0, prod = arena_product(m, l, n)
    wc, wa, wb = g.width(n), g.width(l), g.width(n)
    ld = even(wc + wa + wb)
    P = Parent(max(m, l) + 2, ld, m).put(1, 0, c0).put(1, wc, a).put(1, wc + wa, b).upload()
    C, A, B = P.view(dev, 1, 0, m, n), P.view(dev, 1, wc, m, l), P.view(dev, 1, wc + wa, l, n)
    cur = c0
    for algo, param in ALGOS if m == 300 else [("auto", 0), ("strassen", 1)]:
        dev.mul(A, B, C, accumulate=bool(acc), algo=algo, param=param)
        cur = cur ^ prod if acc else prod   # an accumulating call adds onto what the call before left
        P.check("C (+)= A * B in one arena, %s" % algo, 1, 0, cur)


@pytest.mark.parametrize("nrows,ncols", [(130, 70), (513, 2049)])
def test_transpose_in_one_arena(L, dev, nrows, ncols):
    s = g.random_words(nrows, ncols, 600 + nrows)
    ws, wd = g.width(ncols), g.width(nrows)
    P = Parent(max(nrows, ncols) + 2, even(ws + wd) + 1, nrows).put(1, 0, s)   # an odd ld: 8-byte aligned rows
    P.put(1, ws, g.random_words(ncols, nrows, 601))
    P.upload()
    S, D = P.view(dev, 1, 0, nrows, ncols), P.view(dev, 1, ws, ncols, nrows)
    routed(L, ["gf2_transpose"], lambda: dev.transpose(S, D))
    P.check("D = S^T in one arena", 1, ws, g.o_transpose(s, nrows, ncols))


@pytest.mark.parametrize("nrows,ncols", [(70, 129), (257, 1000)])
def test_add_in_one_arena(L, dev, nrows, ncols):
    a, b = g.random_words(nrows, ncols, 610), g.random_words(nrows, ncols, 611)
    w = g.width(ncols)
    P = Parent(nrows + 2, even(3 * w), nrows).put(1, 0, g.random_words(nrows, ncols, 612)).put(1, w, a).put(1, 2 * w, b).upload()
    C, A, B = P.view(dev, 1, 0, nrows, ncols), P.view(dev, 1, w, nrows, ncols), P.view(dev, 1, 2 * w, nrows, ncols)
    routed(L, ["gf2_xor2d_kernel"], lambda: dev.add(A, B, C=C))
    P.check("C = A + B in one arena", 1, 0, a ^ b)


# ---- gf2_inverse_dev in place -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def square_matrix(n, invertible):
    """the first seed from 1000 + n on whose n x n matrix is (not) invertible, with its inverse"""
    seed = 1000 + n
    while True:
        a = g.random_words(n, n, seed)
        inv = g.o_inverse(a, n)
        if (inv is not None) == invertible:
            a.setflags(write=False)
            return a, inv
        seed += 1000


@pytest.mark.parametrize("invertible", [True, False], ids=["invertible", "singular"])
@pytest.mark.parametrize("n", [65, 200, 300])
def test_inverse_in_place(L, dev, n, invertible):
    """Ainv identical to A: A is copied into scratch before Ainv is written.  A singular A is left unchanged."""
    a, inv = square_matrix(n, invertible)
    P = Parent(n + 2, even(g.width(n)) + 4, n).put(1, 2, a).upload()
    for same_struct in (True, False):
        A = P.view(dev, 1, 2, n, n)
        Ainv = A if same_struct else P.view(dev, 1, 2, n, n)
        singular = ctypes.c_int(7)
        k0 = census(L)
        rc = L.gf2_inverse_dev(ctypes.byref(Ainv.s), ctypes.byref(A.s), ctypes.byref(singular), None)
        assert rc == 0, L.gf2_last_error()
        # [A | pad | I] of 65 and 200 rows is one launch; 300 columns to visit take the blocked elimination
        assert_route(k0, census(L), ["gf2_set_diag_kernel", "gf2_elim_small_kernel" if n <= 200 else "gf2_elim_pivot_kernel"])
        assert singular.value == (0 if invertible else 1)
        P.check("the inverse in place", 1, 2, inv if invertible else None)
        if not invertible:
            break
        # ... and back: the inverse of the inverse, in place again
        assert L.gf2_inverse_dev(ctypes.byref(Ainv.s), ctypes.byref(A.s), ctypes.byref(singular), None) == 0 and singular.value == 0
        P.check("the inverse of the inverse", 1, 2, a)


# ---- gf2_equal_dev ----------------------------------------------------------------------------------------------------------------------

def test_equal_with_one_buffer(L, dev):
    nrows, ncols = 70, 129
    a = g.random_words(nrows, ncols, 700)
    P = Parent(nrows + 2, 6, 9).put(1, 2, a).upload()
    Q = Parent(nrows + 2, 6, 10).put(1, 2, a).upload()
    A, A2, other = P.view(dev, 1, 2, nrows, ncols), P.view(dev, 1, 2, nrows, ncols), Q.view(dev, 1, 2, nrows, ncols)
    assert routed(L, ["gf2_diff_kernel"], lambda: dev.equal(A, A)) and dev.equal(A, A2) and dev.equal(A, other)
    P.buf[1 + 40, 2 + 1] ^= 1 << 17  # one bit, through the buffer both views are cut from
    assert dev.equal(A, A) and dev.equal(A, A2), "both views see the flip"
    assert not dev.equal(A, other)
    assert dev.equal(A, P.view(dev, 2, 2, nrows, ncols)) is False  # overlapping, one row further down: compared, not refused


# ---- every refusal once more, with live buffers -----------------------------------------------------------------------------------------

def test_refusals_touch_nothing(L, dev):
    """-1, the buffer byte-identical afterwards, and nothing allocated (so nothing was launched either: the census agrees)"""
    n, ld = 130, 8
    P = Parent(3 * n, ld, 21).upload()
    Q = Parent(3 * n, ld, 22).upload()
    ref = ctypes.byref
    X = P.view(dev, 0, 0, n, n)          # words 0-2 of rows 0 .. 129
    far = Q.view(dev, 0, 0, n, n)
    placed = [("identical", P.view(dev, 0, 0, n, n)), ("one row in", P.view(dev, 1, 0, n, n)), ("one word in", P.view(dev, 0, 1, n, n)),
              ("its last row is the other's first", P.view(dev, n - 1, 0, n, n)),
              ("another ld", dev.DMat.wrap(P.buf.data_ptr(), n, n, ld + 2, keep=P.buf))]
    bad, rank, flag = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)   # (the solves clear their flag before they look at the matrices)
    perm = (ctypes.c_int * n)(*range(n))
    counts0, k0 = dp.counts(L), census(L)
    calls = 0
    for what, W in placed:
        w, x, f = ref(W.s), ref(X.s), ref(far.s)
        rcs = [L.gf2_mul_dev(w, x, f, acc, algo, 0, None) for acc in (0, 1) for algo in (0, 1, 2, 3)]
        rcs += [L.gf2_mul_dev(w, f, x, acc, 0, 0, None) for acc in (0, 1)]
        rcs += [L.gf2_mul_nt_dev(w, x, f, acc, None) for acc in (0, 1)] + [L.gf2_mul_nt_dev(w, f, x, acc, None) for acc in (0, 1)]
        rcs += [L.gf2_transpose_dev(w, x, None)]
        rcs += [L.gf2_trsm_dev(x, w, upper, right, None) for upper in (0, 1) for right in (0, 1)]
        rcs += [L.gf2_solve_left_dev(x, w, 1, ref(flag), None), L.gf2_pluq_solve_left_dev(x, 0, perm, perm, w, 1, ref(flag), None)]
        if what != "identical":
            rcs += [L.gf2_add_dev(w, x, f, None), L.gf2_add_dev(w, f, x, None), L.gf2_add_dev(w, w, x, None)]
        for rc in rcs:
            assert rc == -1, (what, rcs)
        assert "overlap" in L.gf2_last_error().decode()
        calls += len(rcs)
    # the argument errors: a stride below the row width, a base off the 8-byte grid, a null out-pointer
    thin = dev.DMat.wrap(P.buf.data_ptr(), n, n, 2, keep=P.buf)
    off = dev.DMat.wrap(Q.buf.data_ptr() + 4, n, n, ld, keep=Q.buf)
    for M in (thin, off):
        m = ref(M.s)
        rcs = [L.gf2_mul_dev(m, ref(X.s), ref(far.s), 0, 0, 0, None), L.gf2_add_dev(ref(far.s), m, ref(far.s), None),
               L.gf2_transpose_dev(ref(far.s), m, None), L.gf2_equal_dev(m, ref(far.s), ref(bad), None),
               L.gf2_inverse_dev(ref(far.s), m, ref(bad), None), L.gf2_inverse_dev(m, ref(far.s), ref(bad), None),
               L.gf2_trsm_dev(m, ref(far.s), 0, 0, None), L.gf2_echelonize_dev(m, 1, 0, ref(rank), None, None),
               L.gf2_ple_dev(m, 0, perm, perm, ref(rank), None), L.gf2_apply_p_dev(m, perm, n, 0, 0, None)]
        assert all(rc == -1 for rc in rcs), rcs
        calls += len(rcs)
    assert L.gf2_equal_dev(ref(X.s), ref(far.s), None, None) == -1 and L.gf2_inverse_dev(ref(far.s), ref(X.s), None, None) == -1
    assert L.gf2_echelonize_dev(ref(X.s), 1, 0, None, None, None) == -1
    assert bad.value == 7 and rank.value == 7 and calls > 100
    assert dp.counts(L) == counts0, "a refused call allocated device memory"
    assert census(L) == k0, "a refused call launched a kernel"
    P.check("the buffer of the refused calls")
    Q.check("the other buffer of the refused calls")
