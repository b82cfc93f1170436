"""Device paths past 2^22 rows and past 4 GiB operands, bit for bit.

Two thresholds lie above every other shape of the suite.  (1) A row or column count past 65 536 x 64 = 4 194 304: gf2_transpose_kernel
and gf2_rowparity_kernel put one workgroup per 64 rows into gridDim.y, so these shapes launch with gridDim.y = 65 538.  (2) Operands
larger than 4 GiB: every byte offset past 2^32, in the streaming helpers, the table and wave-per-row kernels, the tile kernel on an A
that must not be packed, the 512-tile transposition and the elimination's row walks.

Shapes (limits_ref.py): R = 4 194 369 rows; big-tall 9 000 001 x 4096 (4.6 GB, byte offset 2^32 at row 8 388 608); big-wide 36 929 x
1 048 640 (4.84 GB, ld 16 386).  Operands are filled on the device from a seed; limits_ref.seeded_words gives any of their rows or word
columns on the CPU without a download.  A result that is small (at most 2^23 rows of at most 256 columns, a transposition of R x <= 127)
is compared in full against the oracle.  A large one is compared on sampled rows (limits_ref.sample_rows: the ends, both sides of each
limit, the last ragged block, 200 drawn rows) against the oracle, and in addition gf2_equal_dev must call it equal to the same operation
done in pieces below both limits (row blocks of at most 2^21 rows and 2 GiB through views of the same buffers) whose sampled rows are
checked too.  gf2_equal_dev itself is pinned first, at these sizes.  Every case asserts through the launch census that the kernel family
it names ran, starts with a call that waits for the device (an error left by an earlier case ends the session) and prints the families
and its wall time.

Four listed shapes go elsewhere under the shipped thresholds and were replaced by the nearest that goes where intended:
  * 16 x R times R x 40 (two wave-per-row passes): any product of 17-64 vectors with rows of 2048 bits and more takes the slab tables;
    gf2_mul_dev reaches the wave-per-row kernel with at most 16 vectors -> 16 x R times R x 16.  (Its second pass is reachable through
    gf2_mul_nt_dev alone, which transposes nothing.)
  * the result side copy of R x 256 times 256 x 1: one to four vectors take the fused product-and-side launch, which transposes
    nothing -> 256 x 5 with A cached on the device (the plain schedule), whose side copy is gf2_transpose_kernel on all R rows;
  * R x 64 x 1 with algo m4rm goes to the tile kernel -> naive only (gf2_narrow_kernel);
  * 33 x 1 048 640 times 1 048 640 x 36 929: the result is 33 rows, the reference is what is large (all of B), so the oracle gets sampled
    word COLUMNS of B (first, last ragged, six drawn) and the pieces split the inner dimension.
With operands of at most 4.84 GB every WORD offset stays below 2^31; it is byte offsets that pass 2^32 here.
What the first run on an MI355X pinned: the HIP runtime accepts gridDim.y = 65 538 at both launch sites (gf2k_transpose, gf2k_rowparity),
every case is bit-exact, and no kernel or launcher needed changing.
The module's name sorts before tests/test_zz_kernel_census.py."""
import concurrent.futures
import ctypes
import functools
import gc
import time

import numpy as np
import pytest

import gf2util as g
import limits_ref as lr
from census_util import assert_route, census
from limits_ref import BIG_TALL, BIG_WIDE, R

pytestmark = pytest.mark.gpu

GIB = 1 << 30


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


@pytest.fixture(scope="module", autouse=True)
def memory(L):
    """the cases hold up to 16 GiB on the device: the module runs when 24 GiB are free, and gives everything back at its end"""
    import torch
    L.gf2_trim()
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * GIB:
        reason = "tests/test_gpu_limits.py needs 24 GiB of free device memory, %.1f GiB are free" % (free / GIB)
        print(reason)
        pytest.skip(reason)
    yield
    gc.collect()
    L.gf2_trim()


class Case:
    """with Case(L, name) as c: starts with a call that waits for the device, c.route(families) asserts the census since the last mark,
    the end prints the families seen and the wall time and returns the case's cached blocks to the driver"""

    def __init__(self, L, name):
        self.L, self.name, self.seen = L, name, []

    def __enter__(self):
        gc.collect()
        if self.L.gf2_trim() != 0:
            msg = self.L.gf2_last_error()
            pytest.exit("the device reports an error left by an earlier case; no further case is started: %s" % (msg.decode() if msg else ""),
                        returncode=3)
        self.t0, self.k0 = time.perf_counter(), census(self.L)
        return self

    def mark(self):
        self.k0 = census(self.L)

    def route(self, families, absent=()):
        k1 = census(self.L)
        assert_route(self.k0, k1, families)
        for f in absent:
            ran = [k for k, v in k1.items() if f in k and v > self.k0.get(k, 0)]
            assert not ran, "route check: %s ran" % ran
        self.seen += [f for f in families if f not in self.seen]
        self.k0 = k1

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            print("limits %s: census saw %s, wall %.2f s" % (self.name, ", ".join(self.seen), time.perf_counter() - self.t0))
        gc.collect()
        return False


def o_mul(a, b, m, l, n):
    """the oracle's product: its row-parity form for narrow results (its table form takes minutes on a long inner dimension)"""
    return (g.o_mul_naive if n <= 64 else g.o_mul_m4rm)(a, b, m, l, n)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d wrong words, first at (row, word) %s" % (what, len(bad), tuple(bad[0]))


def same_rows(dev, M, rows, want, what):
    got = lr.fetch_rows(dev, M, rows)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d wrong words in the sampled rows, first at row %d word %d" % (what, len(bad), rows[bad[0][0]], bad[0][1])


# ---- the references are checked first ---------------------------------------------------------------------------------------------

def test_seeded_rows_on_the_cpu_match_the_generator(L, dev):
    """limits_ref.seeded_words against gf2util.random_words and against what the device generator writes, rows and word columns"""
    with Case(L, "seeded-rows") as c:
        for m, n, seed in ((1000, 200, 5), (77, 64, 6), (513, 1, 7), (300, 4097, 8)):
            full = g.random_words(m, n, seed)
            rows = np.array([0, 1, m // 2, m - 1])
            assert np.array_equal(lr.seeded_words(seed, n, rows), full[rows])
            words = np.array([0, g.width(n) - 1])
            assert np.array_equal(lr.seeded_words(seed, n, np.arange(m), words), full[:, words])
            assert np.array_equal(lr.seeded_matrix(seed, m, n, chunk=100), full)
            M = dev.DMat.random(m, n, seed)
            assert np.array_equal(M.to_words(), full)
            assert np.array_equal(lr.fetch_rows(dev, M, rows), full[rows])
        a, b = g.random_words(9, 1000, 1), g.random_words(1000, 130, 2)
        assert np.array_equal(lr.mul_rows_ref(a, b, 1000), g.o_mul_m4rm(a, b, 9, 1000, 130))
        assert lr.straddle(64, BIG_TALL[0]) == (8388607, 8388608) and lr.straddle(4, 1000) == ()
        for want in (0, R - 1, R - 65, lr.LIMIT_ROWS - 1, lr.LIMIT_ROWS):
            assert want in lr.sample_rows(R, 2, 1)
        assert len(lr.sample_rows(BIG_WIDE[0], 16386, 1)) >= 200 and {32764, 32765} <= set(lr.sample_rows(BIG_WIDE[0], 16386, 1))
        c.route(["gf2_fill_random_kernel"])


@pytest.mark.parametrize("shape", [BIG_TALL, BIG_WIDE], ids=["big-tall", "big-wide"])
def test_the_comparator_sees_one_bit_at_these_sizes(pkg, dev, L, shape):
    """gf2_equal_dev on two equal seeded operands past 4 GiB (big-tall: past 2^22 rows too): one flipped bit in the last valid word of
    the last row, in row 4 194 304, and in the last word below and the first word at byte offset 2^32 makes them different; restored,
    they are equal again"""
    m, n = shape
    with Case(L, "comparator-%dx%d" % shape) as c:
        A, B = dev.DMat.random(m, n, 11), dev.DMat.random(m, n, 11)
        ld, w = A.ld, g.width(n)
        assert m * ld * 8 > lr.LIMIT_BYTES
        assert dev.equal(A, B)
        c.route(["gf2_diff_kernel", "gf2_fill_random_kernel"])
        k = lr.straddle(ld, m)[1]
        first = lr.LIMIT_BYTES // 8 - (k - 1) * ld  # the word of row k - 1 at byte offset 2^32, if that row reaches it (else: word 0 of row k)
        spots = [(m - 1, w - 1, (n - 1) % 64), (0, 0, 0), (k, 0, 5), (k - 1, w - 1, 9)]
        if first < w:
            spots += [(k - 1, first, 3), (k - 1, first - 1, 4)]
        if m > lr.LIMIT_ROWS:
            spots += [(lr.LIMIT_ROWS, 1, 63), (lr.LIMIT_ROWS - 1, w - 1, 0)]
        for r, j, bit in spots:
            lr.flip_bit(pkg, dev, B, r, j, bit)
            assert not dev.equal(A, B), "a flipped bit at row %d word %d went unseen" % (r, j)
            assert not dev.equal(B, A)
            lr.flip_bit(pkg, dev, B, r, j, bit)
            assert dev.equal(A, B), "row %d word %d restored" % (r, j)
        c.route(["gf2_diff_kernel"])


# ---- 1, 2: transpositions with R source rows --------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(R, 1), (R, 64), (R, 127), (1, R), (127, R)])
def test_transpose_dev_past_the_row_limit(dev, L, rows, cols):
    """gf2_transpose_dev below 2^29 bits: the block kernel with gridDim.y = 65 538 (R source rows) and the same count in x (R columns)"""
    assert rows * cols < 1 << 29 and (max(rows, cols) + 63) // 64 == 65538
    with Case(L, "transpose-%dx%d" % (rows, cols)) as c:
        S = dev.DMat.random(rows, cols, 21)
        D = dev.transpose(S)
        got = D.to_words()
        c.route(["gf2_transpose_kernel"], absent=["gf2_transpose512"])
        same(got, g.o_transpose(lr.seeded_matrix(21, rows, cols), rows, cols), "transpose")
        assert dev.equal(dev.transpose(D), S)


def test_host_transpose_past_the_row_limit(pkg, L):
    """mzd_transpose of an R x 4 host matrix (2^24 bits: the device route, which falls back to the host loop silently if it fails)"""
    with Case(L, "mzd_transpose-Rx4") as c:
        s = lr.seeded_matrix(22, R, 4)
        A = pkg.BinMatrix.from_words(s, 4)
        c.mark()
        T = A.transposed()
        c.route(["gf2_transpose_kernel"])
        assert T.nrows() == 4 and T.ncols() == R
        same(T.to_words(), g.o_transpose(s, R, 4), "mzd_transpose")


# ---- 3: row parity with R rows of Bt ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l,family", [(64, "gf2_rowparity_kernelILi1E"), (200, "gf2_rowparity_kernelILi4E")])
def test_mul_nt_past_the_row_limit(dev, L, l, family):
    """gf2_mul_nt_dev with R rows in Bt: one workgroup per 64 output columns, gridDim.y = 65 538; plain and accumulate"""
    with Case(L, "mul_nt-8x%dxR" % l) as c:
        a, c0 = g.random_words(8, l, 31), lr.seeded_matrix(33, 8, R)
        bt = lr.seeded_matrix(32, R, l)
        ref = g.o_transpose(g.o_mul_m4rm(bt, g.o_transpose(a, 8, l), R, l, 8), R, 8)  # A Bt^T = (Bt A^T)^T
        A, Bt = dev.DMat.from_words(a, l), dev.DMat.random(R, l, 32)
        same(dev.mul_nt(A, Bt).to_words(), ref, "mul_nt")
        C = dev.DMat.random(8, R, 33)
        same(dev.mul_nt(A, Bt, C, accumulate=True).to_words(), ref ^ c0, "mul_nt accumulate")
        c.route([family])


# ---- 4: wave per row, B with R rows is transposed ---------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ["naive", "m4rm"])
@pytest.mark.parametrize("m,n", [(8, 8), (16, 16)])
def test_wave_per_row_transposes_a_b_past_the_row_limit(dev, L, m, n, algo):
    with Case(L, "widevec-%dxRx%d-%s" % (m, n, algo)) as c:
        a, b, c0 = lr.seeded_matrix(41, m, R), lr.seeded_matrix(42, R, n), g.random_words(m, n, 43)
        ref = o_mul(a, b, m, R, n)
        A, B = dev.DMat.random(m, R, 41), dev.DMat.random(R, n, 42)
        same(dev.mul(A, B, algo=algo).to_words(), ref, "product")
        c.route(["gf2_widevec_kernel", "gf2_transpose_kernel"])
        C = dev.DMat.from_words(c0, n)
        same(dev.mul(A, B, C, accumulate=True, algo=algo).to_words(), ref ^ c0, "accumulate")
        c.route(["gf2_widevec_kernel", "gf2_transpose_kernel"])


# ---- 5: the result side copy ------------------------------------------------------------------------------------------------------

def test_result_side_copy_past_the_row_limit(pkg, L):
    """the side copy of an R x 5 product (A cached: the plain schedule) is gf2_transpose_kernel on all R rows; mzd_transpose of the
    product, served from it, gives the bits of the default path"""
    with Case(L, "result-side-Rx256x5") as c:
        a, x = lr.seeded_matrix(51, R, 256), g.random_words(256, 5, 52)
        ref = o_mul(a, x, R, 256, 5)
        reft = g.o_transpose(ref, R, 5)
        A, X = pkg.BinMatrix.from_words(a, 256), pkg.BinMatrix.from_words(x, 5)
        A.cache_on_device()
        prev = L.gf2_set_result_side_cols(8)
        try:
            c.mark()
            P = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))
            c.route(["gf2_lpn8_kernel", "gf2_transpose_kernel"])
            T = P.transposed()
            c.route([], absent=["gf2_transpose"])  # served from the side copy
        finally:
            L.gf2_set_result_side_cols(prev)
        same(P.to_words(), ref, "product")
        same(T.to_words(), reft, "transposed product from the side copy")
        P2 = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))
        c.route(["gf2_lpn8_kernel"], absent=["gf2_transpose"])
        T2 = P2.transposed()
        c.route(["gf2_transpose_kernel"])
        same(T2.to_words(), reft, "transposed product by the default path")
        A.uncache()


# ---- 6: every row-parallel family with R rows -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def tall_a(l):
    a = lr.seeded_matrix(61, R, l)
    a.setflags(write=False)
    return a


ROW_PARALLEL = [
    (256, 1, "naive", "gf2_lpnvec_kernel"), (256, 1, "m4rm", "gf2_lpnvec_kernel"), (256, 64, "m4rm", "gf2_lpn8_kernel"),
    (256, 129, "m4rm", "gf2_lpn256_kernel"), (256, 256, "m4rm", "gf2_lpn256_kernel"), (250, 100, "m4rm", "gf2_lpn8_kernel"),
    (64, 1, "naive", "gf2_narrow_kernel"), (705, 1, "naive", "gf2_tallskinny7_kernel"), (705, 1, "m4rm", "gf2_tallskinny7_kernel"),
    (1025, 8, "m4rm", "gf2_tallskinny7_kernel"),
]


@pytest.mark.parametrize("l,n,algo,family", ROW_PARALLEL)
def test_row_parallel_products_past_the_row_limit(dev, L, l, n, algo, family):
    """R x l x n through gf2_mul_dev, plain and accumulate, the whole result against the oracle"""
    with Case(L, "rows-Rx%dx%d-%s" % (l, n, algo)) as c:
        a, b = tall_a(l), g.random_words(l, n, 62)
        ref = o_mul(a, b, R, l, n)
        A, B = dev.DMat.random(R, l, 61), dev.DMat.from_words(b, n)
        same(dev.mul(A, B, algo=algo).to_words(), ref, "product")
        c.route([family])
        C = dev.DMat.random(R, n, 63)
        same(dev.mul(A, B, C, accumulate=True, algo=algo).to_words(), ref ^ lr.seeded_matrix(63, R, n), "accumulate")
        c.route([family])


# ---- 7, 8: products on operands past 4 GiB ----------------------------------------------------------------------------------------

def tall_product(dev, L, c, shape, n, algo, families, absent=()):
    """(m x l past 4 GiB) x (l x n), plain and accumulate: sampled rows against the oracle for the product and for the same product
    done in row blocks below both limits; gf2_equal_dev calls the two equal"""
    m, l = shape
    A = dev.DMat.random(m, l, 71)
    b = g.random_words(l, n, 72)
    B = dev.DMat.from_words(b, n)
    rows = lr.sample_rows(m, A.ld, 7)
    ref = o_mul(lr.seeded_words(71, l, rows), b, len(rows), l, n)
    assert {lr.straddle(A.ld, m)[0], lr.straddle(A.ld, m)[1], m - 1} <= set(rows)
    for acc in (False, True):
        want = ref ^ lr.seeded_words(73, n, rows) if acc else ref
        C, C2 = dev.DMat(m, n), dev.DMat(m, n)
        if acc:
            C.fill_random(73)
            C2.fill_random(73)
        c.mark()
        dev.mul(A, B, C, accumulate=acc, algo=algo)
        c.route(families, absent)
        same_rows(dev, C, rows, want, "product (accumulate=%d)" % acc)
        for r0, r1 in lr.pieces(m, A.ld):
            dev.mul(lr.row_view(dev, A, r0, r1 - r0), B, lr.row_view(dev, C2, r0, r1 - r0), accumulate=acc, algo=algo)
        same_rows(dev, C2, rows, want, "product in row blocks (accumulate=%d)" % acc)
        assert dev.equal(C, C2), "the product and the same product in row blocks differ (accumulate=%d)" % acc
        del C, C2


def test_tile_kernel_on_an_a_past_4gib_that_is_not_packed(dev, L):
    """big-tall x (4096 x 512): plain_plan must not pack A (its copy would pass the tile kernel's 32-bit byte counts)"""
    (m, l), n = BIG_TALL, 512
    with Case(L, "tiles-big-tall-x512") as c:
        out = (ctypes.c_longlong * 9)()
        L.gf2_tile_plan(m, l, n, 1, 0, out)
        packed_copy = ((m + 63) & ~63) * lr.even(g.width(l)) * 8
        assert packed_copy >= lr.LIMIT_BYTES
        assert L.gf2_mul_workspace_bytes(m, l, n, dev.ALGOS["m4rm"], 0) == out[4] < packed_copy  # partial tiles alone: no packed copy
        tall_product(dev, L, c, BIG_TALL, n, "m4rm", ["gf2_m4rm_kernel"], absent=["gf2_packA_kernel"])


def test_slab_tables_on_an_a_past_4gib(dev, L):
    with Case(L, "slab-tables-big-tall-x64") as c:
        tall_product(dev, L, c, BIG_TALL, 64, "m4rm", ["gf2_tallskinny7_kernel"])


def test_wave_per_row_on_an_a_past_4gib(dev, L):
    with Case(L, "widevec-big-wide-x8") as c:
        tall_product(dev, L, c, BIG_WIDE, 8, "m4rm", ["gf2_widevec_kernel", "gf2_transpose_kernel"])


def test_few_rows_transposed_on_a_b_past_4gib(dev, L):
    """33 x 1 048 640 times 1 048 640 x 36 929: B (4.84 GB) is transposed by the 512-tile kernel, the product runs as slab tables on B^T.
    The oracle gets A and sampled word columns of B; the pieces split the inner dimension below 2 GiB of B each"""
    m, (n, l) = 33, BIG_WIDE
    with Case(L, "few-rows-t-33xbig") as c:
        A, B = dev.DMat.random(m, l, 81), dev.DMat.random(l, n, 82)
        assert l * B.ld * 8 > lr.LIMIT_BYTES
        w = g.width(n)
        cols = np.array(sorted({0, w - 1} | set(int(x) for x in np.random.default_rng(8).integers(0, w, size=6))))
        bcols = lr.seeded_words(82, n, np.arange(l), cols)
        ref = lr.mul_rows_ref(lr.seeded_matrix(81, m, l), bcols, l)
        step = lr.PIECE_BYTES // (8 * B.ld) // 64 * 64
        for acc in (False, True):
            c0 = g.random_words(m, n, 83)
            want = ref ^ c0[:, cols] if acc else ref
            C, C2 = (dev.DMat.from_words(c0, n), dev.DMat.from_words(c0, n)) if acc else (dev.DMat(m, n), dev.DMat(m, n))
            c.mark()
            dev.mul(A, B, C, accumulate=acc, algo="m4rm")
            c.route(["gf2_tallskinny7_kernel", "gf2_transpose512_kernel"])
            same(C.to_words()[:, cols], want, "sampled word columns (accumulate=%d)" % acc)
            for k0 in range(0, l, step):
                k1 = min(l, k0 + step)
                dev.mul(dev.DMat.wrap(A.s.data + 8 * (k0 // 64), m, k1 - k0, A.ld, keep=A), lr.row_view(dev, B, k0, k1 - k0), C2,
                        accumulate=acc or k0 > 0, algo="m4rm")
            same(C2.to_words()[:, cols], want, "sampled word columns of the product in slabs (accumulate=%d)" % acc)
            assert dev.equal(C, C2)


# ---- 9: the streaming helpers past 2^32 bytes -------------------------------------------------------------------------------------

BIG = pytest.mark.parametrize("shape", [BIG_WIDE, BIG_TALL], ids=["big-wide", "big-tall"])


@BIG
def test_fill_random_rows_and_blocks_past_4gib(dev, L, shape):
    """gf2_dmat_fill_random against the CPU generator on sampled rows; _rows and _block through views that span more than 4 GiB give
    the same matrix"""
    m, n = shape
    with Case(L, "fill-%dx%d" % shape) as c:
        A, B = dev.DMat.random(m, n, 91), dev.DMat(m, n)
        rows = lr.sample_rows(m, A.ld, 9)
        want = lr.seeded_words(91, n, rows)
        same_rows(dev, A, rows, want, "fill_random")
        for r0, r1 in ((0, 1001), (1001, m)):
            v = lr.row_view(dev, B, r0, r1 - r0)
            dev._lib.check(L.gf2_dmat_fill_random_rows(v._on(None), 91, r0, None), "gf2_dmat_fill_random_rows")
        same_rows(dev, B, rows, want, "fill_random_rows")
        assert dev.equal(A, B)
        B.fill_random(92)
        assert not dev.equal(A, B)
        w0 = g.width(n) // 3
        for r0, r1 in ((0, m // 2), (m // 2, m)):
            for j0, cols in ((0, 64 * w0), (w0, n - 64 * w0)):
                v = lr.row_view(dev, B, r0, r1 - r0, ncols=cols, word0=j0)
                dev._lib.check(L.gf2_dmat_fill_random_block(v._on(None), 91, r0, j0, n, None), "gf2_dmat_fill_random_block")
        same_rows(dev, B, rows, want, "fill_random_block")
        assert dev.equal(A, B)
        c.route(["gf2_fill_random_kernel", "gf2_diff_kernel"])


@BIG
def test_add_past_4gib(dev, L, shape):
    """C = A ^ B: sampled rows against plain XOR; XORing B into C again in row blocks below both limits must give A back everywhere"""
    m, n = shape
    with Case(L, "add-%dx%d" % shape) as c:
        A, B = dev.DMat.random(m, n, 93), dev.DMat.random(m, n, 94)
        rows = lr.sample_rows(m, A.ld, 10)
        a, b = lr.seeded_words(93, n, rows), lr.seeded_words(94, n, rows)
        C = dev.add(A, B)
        c.route(["gf2_xor2d_kernel"])
        same_rows(dev, C, rows, a ^ b, "add")
        assert not dev.equal(C, A)
        for r0, r1 in lr.pieces(m, A.ld):
            Cv = lr.row_view(dev, C, r0, r1 - r0)
            dev.add(Cv, lr.row_view(dev, B, r0, r1 - r0), Cv)
        same_rows(dev, C, rows, a, "add undone in row blocks")
        assert dev.equal(C, A)


@BIG
def test_copy_block_past_4gib(dev, L, shape):
    """gf2_copy_block_dev of the whole matrix: aligned, and into bit offset 37 of a matrix one word wider, copy and XOR"""
    m, n = shape
    with Case(L, "copy-block-%dx%d" % shape) as c:
        A = dev.DMat.random(m, n, 95)
        rows = lr.sample_rows(m, A.ld, 11)
        a = lr.seeded_words(95, n, rows)
        D = dev.DMat.random(m, n, 96)
        dev.copy_block(D, 0, 0, A, 0, 0, m, n)
        c.route(["gf2_copy_block_kernel"])
        same_rows(dev, D, rows, a, "aligned copy")
        assert dev.equal(D, A)
        del D
        gc.collect()
        L.gf2_trim()  # (the wider matrices below cannot reuse its block)
        for acc in (False, True):
            D, D2 = dev.DMat.random(m, n + 64, 97), dev.DMat.random(m, n + 64, 97)
            want = lr.block_at_offset(lr.seeded_words(97, n + 64, rows), a, n, 37, acc)
            dev.copy_block(D, 0, 37, A, 0, 0, m, n, accumulate=acc)
            c.route(["gf2_copy_block_kernel"])
            same_rows(dev, D, rows, want, "block at bit offset 37 (accumulate=%d)" % acc)
            for r0, r1 in lr.pieces(m, D.ld):
                dev.copy_block(D2, r0, 37, A, r0, 0, r1 - r0, n, accumulate=acc)
            same_rows(dev, D2, rows, want, "block at bit offset 37 in row blocks (accumulate=%d)" % acc)
            assert dev.equal(D, D2)
            del D, D2


@BIG
def test_transpose_past_4gib(dev, L, shape):
    """the 512-tile transposition of a source past 4 GiB (big-wide: 2049 x 73 tiles; big-tall: past 2^22 source rows too).  Sampled rows
    of D are word columns of S: 64 rows at a time against the oracle, for D and for D put together from tiles below both limits"""
    m, n = shape
    with Case(L, "transpose-%dx%d" % shape) as c:
        S = dev.DMat.random(m, n, 98)
        D = dev.transpose(S)
        c.route(["gf2_transpose512_kernel"])
        D2 = dev.DMat(n, m)
        w = g.width(n)
        cstep = min(w, lr.PIECE_BYTES // 2 // (8 * D.ld) // 64)  # word columns of S per tile: at most 1 GiB of D's rows
        for r0, r1 in lr.pieces(m, S.ld):
            for j0 in range(0, w, cstep):
                cols = min(n - 64 * j0, 64 * cstep)
                dev.transpose(lr.row_view(dev, S, r0, r1 - r0, ncols=cols, word0=j0),
                              dev.DMat.wrap(D2.s.data + 8 * (64 * j0 * D2.ld + r0 // 64), cols, r1 - r0, D2.ld, keep=D2))
        # sampled rows of D are word columns of S, 64 rows at a time: the ends, both sides of byte offset 2^32 of D, drawn ones where a
        # column of S is short; sampled word columns of D are 64-row blocks of S and cover EVERY row of D: the ends, both sides of row
        # 4 194 304 and of byte offset 2^32 of S, drawn ones
        rng = np.random.default_rng(12)
        groups = sorted({0, w - 1} | {r // 64 for r in lr.straddle(D.ld, n)} | set(int(x) for x in rng.integers(0, w, size=3 if m < 1 << 20 else 0)))
        blocks = sorted({0, (m - 1) // 64} | {r // 64 for r in lr.straddle(S.ld, m)} | ({65535, 65536} if m > lr.LIMIT_ROWS else set())
                        | set(int(x) for x in rng.integers(0, (m + 63) // 64, size=2 if n > 1 << 20 else 8)))

        def rows_of_d(j):
            return g.o_transpose(lr.seeded_words(98, n, np.arange(m), [j]), m, min(64, n - 64 * j))

        def words_of_d(i):
            srows = np.arange(64 * i, min(m, 64 * i + 64))
            return g.o_transpose(lr.seeded_words(98, n, srows), len(srows), n)

        with concurrent.futures.ThreadPoolExecutor(4) as pool:  # (the oracle runs outside the interpreter lock)
            want_rows, want_words = list(pool.map(rows_of_d, groups)), list(pool.map(words_of_d, blocks))
        for j, want in zip(groups, want_rows):
            drows = np.arange(64 * j, 64 * j + len(want))
            same_rows(dev, D, drows, want, "transpose, word column %d of the source" % j)
            same_rows(dev, D2, drows, want, "transpose in tiles, word column %d of the source" % j)
        for i, want in zip(blocks, want_words):
            for M, what in ((D, "transpose"), (D2, "transpose in tiles")):
                got = dev.DMat.wrap(M.s.data + 8 * i, n, min(64, m - 64 * i), M.ld, keep=M).to_words()
                same(got, want, "%s, rows %d.. of the source" % (what, 64 * i))
        assert dev.equal(D, D2)


# ---- 10: elimination past 2^22 rows -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def low_rank_tall():
    m, n, r = R, 130, 70
    a = g.o_mul_m4rm(g.random_words(m, r, 101), g.random_words(r, n, 102), m, r, n)
    a[: m // 2] = 0  # every pivot comes from far down
    ref, rank, piv = g.o_echelonize(a, m, n, full=True)
    for x in (a, ref):
        x.setflags(write=False)
    return a, ref, rank, piv


@pytest.mark.parametrize("full", [True, False], ids=["full", "upper"])
def test_echelonize_past_the_row_limit(dev, L, full):
    """R x 130 of rank 70 with an empty upper half: row walks, flags and pivot search past row 4 194 304"""
    with Case(L, "echelonize-Rx130-%s" % ("full" if full else "upper")) as c:
        a, ref, orank, opiv = low_rank_tall()
        A = dev.DMat.from_words(a, 130)
        c.mark()
        rank, piv = dev.echelonize(A, full=full)
        c.route(["gf2_elim_"])
        assert rank == orank == 70 and piv == opiv
        got = A.to_words()
        if full:
            same(got, ref, "reduced echelon form")
        else:  # upper form: same rank and, reduced on the host, the same reduced form
            again, rank2, _ = g.o_echelonize(got, R, 130, full=True)
            assert rank2 == rank
            same(again, ref, "upper form, reduced on the host")


def test_solve_left_past_the_row_limit(dev, L):
    """R equations in 64 unknowns, 3 right-hand sides (consistent: B = A X0)"""
    with Case(L, "solve_left-Rx64x3") as c:
        a, x0 = lr.seeded_matrix(103, R, 64), g.random_words(64, 3, 104)
        b = o_mul(a, x0, R, 64, 3)
        want, ok = g.o_solve_left(a, R, 64, b, R, 3)
        assert ok and np.array_equal(want[:64], x0)
        A, B = dev.DMat.random(R, 64, 103), dev.DMat.from_words(b, 3)
        c.mark()
        assert dev.solve_left(A, B)
        c.route(["gf2_elim_"])
        same(B.to_words(), want, "solution")
        aref, rank, _ = g.o_echelonize(a, R, 64, full=True)
        assert rank == 64
        same(A.to_words(), aref, "A's reduced echelon form")
