"""GPU parity tests: the HIP path, called through the C ABI (mzd_* entry points and the
device-resident gf2_* API), against the CPU oracle, the committed golden vectors and
size-independent algebraic properties.  Bit-exact everywhere (integer work)."""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

import gf2util as g

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _host_mul(pkg, a, b, m, l, n, strategy):
    pkg.set_mul_strategy(strategy)
    try:
        A = pkg.BinMatrix.from_words(a, l)
        B = pkg.BinMatrix.from_words(b, n)
        C = A * B
        assert C.nrows() == m and C.ncols() == n
        return C.to_words()
    finally:
        pkg.set_mul_strategy("strassen")


# ---- the reference's own known answers (binary_matrix.rs:662-686) ------------------------------

def test_ref_mul_identity(pkg):
    m1, m2, m3 = (pkg.BinMatrix.identity(8) for _ in range(3))
    assert (m1 * m2) == m3


def test_ref_vecmul(pkg):
    m1 = pkg.BinMatrix.identity(10)
    binvec = pkg.BinVector.from_elem(10, True)
    assert (m1 * binvec) == binvec
    assert (binvec * m1) == binvec
    m1 = pkg.BinMatrix.random(10, 3)
    assert len(binvec * m1) == 3


@pytest.mark.parametrize("strategy", ["strassen", "m4rm", "naive"])
def test_identity_products_all_strategies(pkg, strategy):
    pkg.set_mul_strategy(strategy)
    try:
        for n in (1, 8, 63, 64, 65, 200, 1000):
            a = pkg.BinMatrix.random(n, n)
            i = pkg.BinMatrix.identity(n)
            assert (a * i) == a and (i * a) == a
    finally:
        pkg.set_mul_strategy("strassen")


# ---- golden vectors -------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))), ids=os.path.basename)
@pytest.mark.parametrize("strategy", ["strassen", "m4rm", "naive"])
def test_golden_full(pkg, path, strategy):
    z = np.load(path)
    m, l, n = (int(x) for x in z["dims"])
    c = _host_mul(pkg, z["a"], z["b"], m, l, n, strategy)
    assert np.array_equal(c, z["c"])


def test_golden_digests(pkg, dev):
    with open(os.path.join(GOLDEN, "digests.json")) as f:
        dig = json.load(f)
    for name, d in sorted(dig.items()):
        m, l, n = d["m"], d["l"], d["n"]
        A = dev.DMat.random(m, l, d["seed_a"])
        B = dev.DMat.random(l, n, d["seed_b"])
        for algo in ("m4rm", "strassen", "naive"):
            c = dev.mul(A, B, algo=algo).to_words()
            assert hashlib.sha256(c.tobytes()).hexdigest() == d["sha256_c"], (name, algo)


def _large_digests():
    with open(os.path.join(GOLDEN, "digests_large.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("v", [1, 64, 128, 256])
def test_full_size_config5_lpn_digests(pkg, dev, v):
    """BASELINE config 5 at its stated size, 2^20 x 256 times 256 x V (mul_slice / mzd_mul_naive path,
    binary_matrix.rs:416-431, mzd.rs:152): the device product through all three entry points' algorithms must hash to
    the digest of the independent numpy product (tests/golden/make_golden_large.py)."""
    d = _large_digests()["lpn_1048576x256x%d" % v]
    m, l, n = d["m"], d["l"], d["n"]
    assert (m, l, n) == (1 << 20, 256, v)
    A, B = dev.DMat.random(m, l, d["seed_a"]), dev.DMat.random(l, n, d["seed_b"])
    for algo in ("naive", "m4rm", "strassen"):
        c = dev.mul(A, B, algo=algo).to_words()
        assert hashlib.sha256(c.tobytes()).hexdigest() == d["sha256_c"], (v, algo)
    del A, B
    if v == 1:  # and once through the friendly layer exactly as the reference's `&A * &v` does it (host mzd_t, mul_slice)
        a = g.random_words(m, l, d["seed_a"])
        x = g.random_words(l, 1, d["seed_b"])  # 256 x 1: one word per row, bit 0
        vec = pkg.BinVector.from_bools([bool(int(w) & 1) for w in x[:, 0]])
        got = pkg.BinMatrix.from_words(a, l) * vec
        assert len(got) == m
        bits = np.unpackbits(got.get_storage().view(np.uint8), bitorder="little")[:m].reshape(m, 1)
        assert hashlib.sha256(g.bits_to_words(bits).tobytes()).hexdigest() == d["sha256_c"]


@pytest.mark.parametrize("n", [32768, 65536])
def test_full_size_square_digests(dev, n):
    """BASELINE configs 3 and 4 (single-GPU form) at full size: sha256 of the whole product, Strassen-over-M4RM (auto)
    and M4RM only, against the digest written by tests/golden/make_golden_large.py (oracle_mul_fast, itself cross-checked
    on sampled rows against plain M4RM and the independent numpy product) -- BASELINE.md section 3's parity gate."""
    d = _large_digests()["sq_%d" % n]
    A, B = dev.DMat.random(n, n, d["seed_a"]), dev.DMat.random(n, n, d["seed_b"])
    C = dev.DMat(n, n)
    rows = d["sample_rows"]
    for algo in ("auto", "m4rm"):
        c = dev.mul(A, B, C=C, algo=algo).to_words()
        assert hashlib.sha256(np.ascontiguousarray(c[rows]).tobytes()).hexdigest() == d["sample_rows_sha256"], (n, algo, "rows")
        assert hashlib.sha256(c.tobytes()).hexdigest() == d["sha256_c"], (n, algo)
        del c
    del A, B, C
    assert dev._lib.lib().gf2_trim() == 0


# ---- device generator == oracle generator ---------------------------------------------------------

def test_device_random_matches_oracle(dev):
    for (r, c) in [(1, 1), (7, 63), (65, 130), (300, 1000)]:
        assert np.array_equal(dev.DMat.random(r, c, 99).to_words(), g.random_words(r, c, 99))


def test_device_random_blocks_match_full_matrix(dev):
    """Row-block and column-panel shards of the seeded matrix (multi-GPU layout) equal slices of the full one."""
    from m4ri_rust_amd import sharded
    full = g.random_words(200, 512, 77)
    blk = dev.DMat(64, 512)
    sharded.fill_row_block(blk, 77, 100)
    assert np.array_equal(blk.to_words(), full[100:164])
    pan = dev.DMat(200, 128)
    sharded.fill_block(pan, 77, 0, 4, 512)
    assert np.array_equal(pan.to_words(), full[:, 4:6])


# ---- random shapes against the oracle -------------------------------------------------------------

SHAPES = [(1, 1, 1), (3, 5, 7), (64, 64, 64), (65, 65, 65), (127, 129, 63), (1, 300, 500), (9, 300, 500),
          (500, 1, 300), (257, 2049, 33), (1025, 70, 2049), (1300, 900, 4100), (2048, 2048, 2048), (300, 4096, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_vs_oracle(pkg, shape):
    m, l, n = shape
    a, b = g.random_words(m, l, 11), g.random_words(l, n, 12)
    ref = g.o_mul_m4rm(a, b, m, l, n)
    for strategy in ("strassen", "m4rm", "naive"):
        assert np.array_equal(_host_mul(pkg, a, b, m, l, n, strategy), ref), strategy


def test_addmul_and_prealloc(pkg):
    L = pkg._lib.lib()
    m, l, n = 130, 200, 190
    a, b, c0 = g.random_words(m, l, 1), g.random_words(l, n, 2), g.random_words(m, n, 3)
    prod = g.o_mul_m4rm(a, b, m, l, n)
    A, B = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n)
    for fn, extra in ((L.mzd_addmul_m4rm, (0,)), (L.mzd_addmul, (0,)), (L.mzd_addmul_naive, ())):
        C = pkg.BinMatrix.from_words(c0, n)
        r = fn(C.mzd, A.mzd, B.mzd, *extra)
        assert r and np.array_equal(C.to_words(), c0 ^ prod)
    for fn, extra in ((L.mzd_mul_m4rm, (0,)), (L.mzd_mul, (0,)), (L.mzd_mul_naive, ())):
        C = pkg.BinMatrix.from_words(c0, n)  # preallocated, overwritten
        r = fn(C.mzd, A.mzd, B.mzd, *extra)
        assert r and np.array_equal(C.to_words(), prod)


def test_mul_naive_t_and_va(pkg):
    L = pkg._lib.lib()
    m, l, n = 300, 256, 70
    a, b = g.random_words(m, l, 5), g.random_words(l, n, 6)
    prod = g.o_mul_naive(a, b, m, l, n)
    A = pkg.BinMatrix.from_words(a, l)
    Bt = pkg.BinMatrix.from_words(g.o_transpose(b, l, n), l)
    C = pkg.BinMatrix.from_words(g.random_words(m, n, 7), n)
    assert L._mzd_mul_naive(C.mzd, A.mzd, Bt.mzd, 1) and np.array_equal(C.to_words(), prod)
    c0 = C.to_words()
    assert L._mzd_mul_naive(C.mzd, A.mzd, Bt.mzd, 0) and np.array_equal(C.to_words(), c0 ^ prod)
    # v * A
    v = g.random_words(1, m, 8)
    V = pkg.BinMatrix.from_words(v, m)
    Am = pkg.BinMatrix.from_words(a, l)
    ref = g.o_mul_m4rm(v, a, 1, m, l)
    C = pkg.BinMatrix.zero(1, l)
    assert L._mzd_mul_va(C.mzd, V.mzd, Am.mzd, 1) and np.array_equal(C.to_words(), ref)
    assert L._mzd_mul_va(C.mzd, V.mzd, Am.mzd, 0) and not C.to_words().any()


def test_windows(pkg):
    L = pkg._lib.lib()
    big = pkg.BinMatrix.from_words(g.random_words(300, 500, 21), 500)
    bw = big.to_words()
    W = L.mzd_init_window(big.mzd, 10, 64, 210, 64 + 130)  # 200 x 130 window, ragged tail
    B = pkg.BinMatrix.from_words(g.random_words(130, 77, 22), 77)
    C = L.mzd_mul_m4rm(None, W, B.mzd, 0)
    sub = g.bits_to_words(g.words_to_bits(bw, 500)[10:210, 64:194])
    ref = g.o_mul_m4rm(sub, B.to_words(), 200, 130, 77)
    assert np.array_equal(pkg.BinMatrix(C).to_words(), ref)
    # window as destination: the parent's bits outside the window must survive
    dst = pkg.BinMatrix.from_words(g.random_words(250, 300, 23), 300)
    before = g.words_to_bits(dst.to_words(), 300)
    Wd = L.mzd_init_window(dst.mzd, 20, 128, 220, 128 + 77)
    assert L.mzd_mul_m4rm(Wd, W, B.mzd, 0)
    after = g.words_to_bits(dst.to_words(), 300)
    expect = before.copy()
    expect[20:220, 128:205] = g.words_to_bits(ref, 77)
    assert np.array_equal(after, expect)
    L.mzd_free(W)
    L.mzd_free(Wd)


def test_matrix_vector_lpn(pkg):
    """A (2^k x 256) * v: the mul_slice path (binary_matrix.rs:416-431,528-542)."""
    m, l = 5000, 256
    a = g.random_words(m, l, 3)
    A = pkg.BinMatrix.from_words(a, l)
    v = pkg.BinVector(g.random_words(1, l, 4)[0], l)
    res = A * v
    ref = g.o_mul_naive(a, g.o_transpose(v.get_storage().reshape(1, -1), 1, l), m, l, 1)
    assert len(res) == m
    assert np.array_equal(res.get_storage(), g.o_transpose(ref, m, 1)[0])


# ---- device-resident API, larger sizes ------------------------------------------------------------

def test_dev_mul_4096_vs_oracle(dev):
    n = 4096
    a, b = g.random_words(n, n, 1), g.random_words(n, n, 2)
    ref = g.o_mul_fast(a, b, n, n, n)
    A, B = dev.DMat.random(n, n, 1), dev.DMat.random(n, n, 2)
    for algo, param in (("m4rm", 0), ("strassen", 1), ("strassen", 2), ("strassen", 3), ("auto", 0)):
        assert np.array_equal(dev.mul(A, B, algo=algo, param=param).to_words(), ref), (algo, param)


def test_dev_accumulate_and_nt(dev):
    m, l, n = 1500, 2000, 2500
    A, B, C0 = dev.DMat.random(m, l, 1), dev.DMat.random(l, n, 2), dev.DMat.random(m, n, 3)
    P = dev.mul(A, B, algo="m4rm")
    C = dev.add(C0, C0)  # zero
    C = dev.add(C, C0)   # copy of C0
    dev.mul(A, B, C=C, accumulate=True, algo="m4rm")
    assert dev.equal(C, dev.add(C0, P))
    Bt = dev.transpose(B)
    assert dev.equal(dev.transpose(Bt), B)
    small_n = 64
    B2 = dev.DMat.random(l, small_n, 5)
    assert dev.equal(dev.mul_nt(A, dev.transpose(B2)), dev.mul(A, B2, algo="m4rm"))


def test_dev_transpose_vs_oracle(dev):
    for (r, c) in [(1, 1), (64, 64), (65, 63), (300, 1000), (1000, 1)]:
        w = g.random_words(r, c, 17)
        assert np.array_equal(dev.transpose(dev.DMat.from_words(w, c)).to_words(), g.o_transpose(w, r, c))


@pytest.mark.parametrize("r,c", [(20000, 30001), (32768, 16448), (9000, 61000), (70001, 7700), (512, 1 << 20), (1 << 20, 513)])
def test_dev_transpose_large_tiles(dev, r, c):
    """From 2^29 bits on the transposition takes 512 x 512-bit tiles whose order over the workgroups is scrambled on purpose (4 x 4
    tile blocks per XCD inside 16 x 8 super-tiles, super-tiles walked diagonally, the XCD's place rotating: gf2_transpose512_kernel):
    ragged edges in both directions, fewer tiles than one super-tile in either direction, strided operands; the oracle's bits."""
    assert r * c >= 1 << 29
    w = g.random_words(r, c, 23)
    S = dev.DMat.from_words(w, c)
    T = dev.transpose(S)
    ref = g.o_transpose(w, r, c)
    assert np.array_equal(T.to_words(), ref)
    del ref, w
    assert dev.equal(dev.transpose(T), S)


@pytest.mark.parametrize("n,levels", [(8192, 1), (16384, 2)])
def test_dev_strassen_equals_m4rm_large(dev, n, levels):
    A, B = dev.DMat.random(n, n, 1), dev.DMat.random(n, n, 2)
    P0 = dev.mul(A, B, algo="m4rm")
    P1 = dev.mul(A, B, algo="strassen", param=levels)
    assert dev.equal(P0, P1)
    # spot-check 64 random rows of the product against the oracle's row-vector product
    rng = np.random.default_rng(5)
    rows = np.sort(rng.choice(n, size=8, replace=False))
    a = g.random_words(n, n, 1)[rows]
    b = g.random_words(n, n, 2)
    ref = g.o_mul_m4rm(np.ascontiguousarray(a), b, len(rows), n, n)
    assert np.array_equal(P1.to_words()[rows], ref)


@pytest.mark.parametrize("m,l,n,levels", [(5120, 1536, 2560, 2), (1280, 2048, 1024, 2), (8704, 4096, 3072, 3), (4096, 8192, 512, 2)])
def test_strassen_packed_leaves(dev, m, l, n, levels):
    """With >= 2 levels the last split pass hands the A leaves to the tile kernel in its row-group-packed layout (64 rows side
    by side per 64-bit column).  Leaf heights that are multiples of 64 but not of the tile height, few-column leaves and an
    odd level count (single-level pass first): all must equal plain M4RM and the oracle on sampled rows."""
    A, B = dev.DMat.random(m, l, 11), dev.DMat.random(l, n, 12)
    P0 = dev.mul(A, B, algo="m4rm")
    P1 = dev.mul(A, B, algo="strassen", param=levels)
    assert dev.equal(P0, P1)
    C = dev.DMat.random(m, n, 13)
    c0 = C.to_words().copy()
    dev.mul(A, B, C, accumulate=True, algo="strassen", param=levels)
    assert np.array_equal(C.to_words(), c0 ^ P0.to_words())
    rows = np.array([0, 63, 64, m // 2 + 1, m - 65, m - 1])
    a = g.random_words(m, l, 11)[rows]
    ref = g.o_mul_m4rm(np.ascontiguousarray(a), g.random_words(l, n, 12), len(rows), l, n)
    assert np.array_equal(P1.to_words()[rows], ref)


def test_packed_tile_paths_ragged(dev):
    """m >= 2048 and n >= 1024: the plain product packs A and runs the paired tile kernels (one row per lane, 2048 x 1024 or
    4096 x 512 tiles).  Ragged rows, inner dimensions from a few bits to a few thousand, ragged column tiles, accumulate:
    bit-exact against the oracle (tools/fuzz_tiles.py is the long form)."""
    rng = np.random.default_rng(21)
    shapes = [(2048, 1, 1024), (2049, 31, 1025), (4097, 33, 1100), (2500, 64, 2049), (6000, 65, 1536), (9300, 129, 1030),
              (4096, 1000, 4096), (5003, 2111, 3001)]
    shapes += [(int(rng.integers(2048, 9000)), int(rng.integers(1, 2500)), int(rng.integers(1024, 5000))) for _ in range(4)]
    for it, (m, l, n) in enumerate(shapes):
        a, b = g.random_words(m, l, 500 + it), g.random_words(l, n, 600 + it)
        ref = g.o_mul_m4rm(a, b, m, l, n)
        A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
        assert np.array_equal(dev.mul(A, B, algo="m4rm").to_words(), ref), (m, l, n)
        assert np.array_equal(dev.mul(A, B, algo="auto").to_words(), ref), (m, l, n)
        c0 = g.random_words(m, n, 700 + it)
        C = dev.DMat.from_words(c0, n)
        dev.mul(A, B, C, accumulate=True, algo="m4rm")
        assert np.array_equal(C.to_words(), c0 ^ ref), (m, l, n)


def test_packed_plain_product_2gib_operand(dev):
    """A plain product whose packed copy of A is ~2 GiB (the tile kernels' 32-bit buffer descriptors run up to their sign bit):
    linearity in B, and a 2000-row window of A (below the packing threshold, other kernel path) gives the same rows."""
    m, l, n = 131072, 131072 - 64, 1024 + 37
    A, B, B2 = dev.DMat.random(m, l, 1), dev.DMat.random(l, n, 2), dev.DMat.random(l, n, 3)
    C1 = dev.mul(A, B, algo="m4rm")
    assert dev.equal(dev.mul(A, dev.add(B, B2), algo="m4rm"), dev.add(C1, dev.mul(A, B2, algo="m4rm")))
    r0, rows = 70000, 2000
    Aw = dev.DMat.from_words(A.to_words()[r0:r0 + rows], l)
    assert np.array_equal(dev.mul(Aw, B, algo="m4rm").to_words(), C1.to_words()[r0:r0 + rows])


@pytest.mark.parametrize("plan", [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0],
                         ids=["four_equal_slabs", "growing_slabs", "two_slabs", "two_row_groups_x_four_slabs", "two_row_groups_x_two_slabs", "fine_then_halves",
                              "fine_then_quarters", "growing_then_halves", "quarters_then_halves", "fine_slabs", "fine_then_whole", "by_the_model"])
@pytest.mark.parametrize("shape", [(16384, 16384, 16384 + 77), (16384 + 256, 32768, 8192 + 64)], ids=lambda s_: "x".join(map(str, s_)))
def test_host_product_pipelined_over_slabs_of_the_inner_dimension(pkg, dev, shape, plan, monkeypatch):
    """Round 5: large host products may run as C ^= A[:, K] B[K, :] over slabs K of the inner dimension (A's slab uploaded by a 2-D
    copy, B's rows contiguous), the last slab in four row blocks whose rows of C are downloaded one by one.  Every schedule
    (M4RI_HIP_HOST_PLAN, read per call) gives the bits of the device-resident product; B cached on the device is borrowed, not uploaded;
    the default strategies of the friendly layer all reach it."""
    m, l, n = shape
    monkeypatch.setenv("M4RI_HIP_HOST_PLAN", str(plan))
    A, B = pkg.BinMatrix.random(m, l), pkg.BinMatrix.random(l, n)
    a, b = A.to_words(), B.to_words()
    ref = dev.mul(dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)).to_words()
    Lc = pkg._lib.lib()
    for _ in range(2):  # back to back: streams, events and pooled blocks are reused
        assert np.array_equal((A * B).to_words(), ref)
    assert np.array_equal(pkg.BinMatrix(Lc.mzd_mul_m4rm(None, A.mzd, B.mzd, 0)).to_words(), ref)
    Cp = pkg.BinMatrix.random(m, n)  # a preallocated destination is overwritten, not accumulated into
    assert Lc.mzd_mul(Cp.mzd, A.mzd, B.mzd, 0) and np.array_equal(Cp.to_words(), ref)
    B.cache_on_device()
    assert np.array_equal((A * B).to_words(), ref)
    B.uncache()
    rows = np.array([0, 4095, 4096, m // 2, m - 1])
    assert np.array_equal(ref[rows], g.o_mul_m4rm(np.ascontiguousarray(a[rows]), b, len(rows), l, n))


@pytest.mark.parametrize("l", [16384 + 192, 16384], ids=["whole_B", "B_in_two_halves"])
def test_host_product_pipelined_over_row_blocks(pkg, dev, l):
    """Host products with >= 16384 rows are pipelined over four row blocks of A and C and, when the inner dimension allows,
    two halves of it (uploads, products and downloads on three streams).  Same bits as the device-resident product; ragged
    column counts; back-to-back calls reuse the streams and events."""
    m, n = 16384, 16384 + 77
    A, B = pkg.BinMatrix.random(m, l), pkg.BinMatrix.random(l, n)
    a, b = A.to_words(), B.to_words()
    ref = dev.mul(dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)).to_words()
    for _ in range(2):
        assert np.array_equal((A * B).to_words(), ref)
    Lc = pkg._lib.lib()
    for fn in (Lc.mzd_mul_m4rm, Lc.mzd_mul):
        assert np.array_equal(pkg.BinMatrix(fn(None, A.mzd, B.mzd, 0)).to_words(), ref)
    assert np.array_equal(pkg.BinMatrix(Lc.mzd_mul_naive(None, A.mzd, B.mzd)).to_words(), ref)
    rows = np.array([0, 4095, 4096, 8191, 12288, m - 1])
    assert np.array_equal(ref[rows], g.o_mul_m4rm(np.ascontiguousarray(a[rows]), b, len(rows), l, n))
    # three threads at once (every thread has its own pair of streams and events)
    import threading
    L, bad = pkg._lib.lib(), []

    def worker():
        c = L.mzd_mul(None, A.mzd, B.mzd, 0)
        if not c or not np.array_equal(pkg.BinMatrix(c).to_words(), ref):
            bad.append(1)

    ts = [threading.Thread(target=worker) for _ in range(3)]
    for t_ in ts:
        t_.start()
    for t_ in ts:
        t_.join()
    assert not bad
    # a row count the blocks do not divide takes the unpipelined route
    A2 = pkg.BinMatrix.random(m + 64, l)
    ref2 = dev.mul(dev.DMat.from_words(A2.to_words(), l), dev.DMat.from_words(b, n)).to_words()
    assert np.array_equal((A2 * B).to_words(), ref2)


def test_algebraic_identities_on_random_shapes(dev):
    """(AB)^T = B^T A^T, (AB)C = A(BC), A(B + B') = AB + AB', A I = A -- on seeded random shapes through every
    algorithm selector, device resident (each identity mixes kernels: tile / tall-skinny / narrow / v*A, transpose, XOR)."""
    rng = np.random.default_rng(77)
    for it in range(12):
        m, l, n, k = (int(rng.choice([1, 7, 64, 65, 300, 1000, 2048, 3000, 4500])) for _ in range(4))
        A, B, B2, C = dev.DMat.random(m, l, 4 * it), dev.DMat.random(l, n, 4 * it + 1), dev.DMat.random(l, n, 4 * it + 2), dev.DMat.random(n, k, 4 * it + 3)
        algo = ("auto", "m4rm", "naive")[it % 3]
        AB = dev.mul(A, B, algo=algo)
        assert dev.equal(dev.transpose(AB), dev.mul(dev.transpose(B), dev.transpose(A), algo=algo)), ("transpose", m, l, n)
        assert dev.equal(dev.mul(AB, C, algo=algo), dev.mul(A, dev.mul(B, C, algo=algo), algo=algo)), ("associativity", m, l, n, k)
        assert dev.equal(dev.mul(A, dev.add(B, B2), algo=algo), dev.add(AB, dev.mul(A, B2, algo=algo))), ("distributivity", m, l, n)
        I = dev.DMat.from_words(g.bits_to_words(np.eye(l, dtype=np.uint8)), l)
        assert dev.equal(dev.mul(A, I, algo=algo), A), ("identity", m, l)


def test_dev_properties_full_size(dev):
    """Size-independent properties at a BASELINE config size (32768): linearity in B and
    associativity with a vector, (A*B)*x == A*(B*x)."""
    n = 32768
    A, B, B2 = dev.DMat.random(n, n, 1), dev.DMat.random(n, n, 2), dev.DMat.random(n, n, 3)
    P = dev.mul(A, B)           # auto: Strassen over M4RM
    P2 = dev.mul(A, B2)
    S = dev.mul(A, dev.add(B, B2))
    assert dev.equal(S, dev.add(P, P2))
    x = dev.DMat.random(n, 64, 4)
    assert dev.equal(dev.mul(P, x, algo="m4rm"), dev.mul(A, dev.mul(B, x, algo="m4rm"), algo="m4rm"))
    I = dev.DMat(n, n)
    from m4ri_rust_amd import BinMatrix
    I = dev.DMat.from_host(BinMatrix.identity(n))
    assert dev.equal(dev.mul(A, I), A) and dev.equal(dev.mul(I, A, algo="m4rm"), A)


# ---- one process, several devices: row shares of A and C (SURVEY.md section 8e behind the C ABI) ----------

@pytest.mark.parametrize("m,l,n,shares", [(5000, 3000, 2100, 3), (16384, 4096, 4096, 2), (1000, 700, 900, 4), (70000, 256, 64, 2),
                                          (3, 100, 100, 2)])
def test_multi_device_shares_through_c_abi(pkg, dev, monkeypatch, m, l, n, shares):
    """gf2_mul_multi and the automatic form of the drop-in entry points (M4RI_HIP_DEVICES): the rows of A and C are
    divided among device shares, one worker thread each.  With one GPU visible the shares all run on device 0 (an ordinal
    may repeat), with several they spread over them: same code path, same bits as the oracle."""
    import ctypes
    L = pkg._lib.lib()
    nvis = dev.device_count()
    devices = [i % nvis for i in range(shares)]
    a, b = g.random_words(m, l, 41), g.random_words(l, n, 42)
    ref = g.o_mul_m4rm(a, b, m, l, n)
    A, B = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n)
    arr = (ctypes.c_int * shares)(*devices)
    for algo in (dev.ALGO_AUTO, dev.ALGO_M4RM, dev.ALGO_NAIVE):
        c = L.gf2_mul_multi(None, A.mzd, B.mzd, algo, 0, arr, shares)
        assert c, "NULL product"
        assert np.array_equal(pkg.BinMatrix(c).to_words(), ref), algo
    # preallocated destination
    Cp = pkg.BinMatrix.random(m, n)
    assert L.gf2_mul_multi(Cp.mzd, A.mzd, B.mzd, dev.ALGO_AUTO, 0, arr, shares)
    assert np.array_equal(Cp.to_words(), ref)
    # the drop-in entry points with a device list from the environment, accumulate form included
    monkeypatch.setenv("M4RI_HIP_DEVICES", ",".join(str(d) for d in devices))
    for fn in (L.mzd_mul, L.mzd_mul_m4rm):
        c = fn(None, A.mzd, B.mzd, 0)
        assert c and np.array_equal(pkg.BinMatrix(c).to_words(), ref)
    c0 = g.random_words(m, n, 43)
    Cacc = pkg.BinMatrix.from_words(c0, n)
    assert L.mzd_addmul(Cacc.mzd, A.mzd, B.mzd, 0)
    assert np.array_equal(Cacc.to_words(), c0 ^ ref)
    # a bad ordinal is refused, not dereferenced
    bad = (ctypes.c_int * 2)(0, nvis)
    assert not L.gf2_mul_multi(None, A.mzd, B.mzd, dev.ALGO_AUTO, 0, bad, 2)


def test_multi_device_two_distinct_devices(pkg, dev, monkeypatch):
    """The code that only matters ACROSS devices -- hipSetDevice per worker thread, blocks freed into another device's pool,
    portable pinned host blocks read by device 1, the pipelined share (>= 16384 rows) on each -- with devices = [0, 1].
    Skipped on a one-GPU box (there the shares repeat ordinal 0, test_multi_device_shares_through_c_abi)."""
    import ctypes
    if dev.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    L = pkg._lib.lib()
    arr = (ctypes.c_int * 2)(0, 1)
    for (m, l, n) in [(5000, 3000, 2100), (32768, 8192, 4096)]:
        a, b = g.random_words(m, l, 81), g.random_words(l, n, 82)
        ref = g.o_mul_fast(a, b, m, l, n) if m * l * n > 1 << 34 else g.o_mul_m4rm(a, b, m, l, n)
        A, B = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n)
        for algo in (dev.ALGO_AUTO, dev.ALGO_M4RM):
            c = L.gf2_mul_multi(None, A.mzd, B.mzd, algo, 0, arr, 2)
            assert c and np.array_equal(pkg.BinMatrix(c).to_words(), ref), (m, l, n, algo)
        # everything pinned to device 1 from the environment: product, elimination and the operand cache run there
        monkeypatch.setenv("M4RI_HIP_DEVICES", "1")
        c = L.mzd_mul(None, A.mzd, B.mzd, 0)
        assert c and np.array_equal(pkg.BinMatrix(c).to_words(), ref)
        A.cache_on_device()
        c = L.mzd_mul(None, A.mzd, B.mzd, 0)
        assert c and np.array_equal(pkg.BinMatrix(c).to_words(), ref)
        A.uncache()
        monkeypatch.delenv("M4RI_HIP_DEVICES")


def test_pinned_single_ordinal_keeps_one_stream_per_device(pkg, dev, monkeypatch):
    """M4RI_HIP_DEVICES = one ordinal pins products, elimination, transpose and the operand cache of the host entry points to
    that device, and a thread that alternates between pinned and unpinned calls gets the same private stream (and its
    arenas) back each time: the library's device memory must not grow with the number of alternations (round-2 advice)."""
    L = pkg._lib.lib()
    n = 2048
    a, b = g.random_words(n, n, 91), g.random_words(n, n, 92)
    ref = g.o_mul_m4rm(a, b, n, n, n)
    A, B = pkg.BinMatrix.from_words(a, n), pkg.BinMatrix.from_words(b, n)
    import torch
    last = dev.device_count() - 1

    def round_trip():
        monkeypatch.setenv("M4RI_HIP_DEVICES", str(last))
        c = L.mzd_mul_m4rm(None, A.mzd, B.mzd, 0)
        assert c and np.array_equal(pkg.BinMatrix(c).to_words(), ref)
        assert pkg.BinMatrix.from_words(a, n).rank() == g.o_echelonize(a, n, n)[1]
        A.cache_on_device()
        c = L.mzd_mul(None, A.mzd, B.mzd, 0)
        assert c and np.array_equal(pkg.BinMatrix(c).to_words(), ref)
        A.uncache()
        monkeypatch.delenv("M4RI_HIP_DEVICES")
        assert pkg.BinMatrix.from_words(a, n).rank() == g.o_echelonize(a, n, n)[1]

    for _ in range(2):
        round_trip()
    torch.cuda.synchronize()
    free0 = [torch.cuda.mem_get_info(d)[0] for d in range(dev.device_count())]
    for _ in range(6):
        round_trip()
    torch.cuda.synchronize()
    free1 = [torch.cuda.mem_get_info(d)[0] for d in range(dev.device_count())]
    assert all(f0 - f1 < (64 << 20) for f0, f1 in zip(free0, free1)), (free0, free1)


def test_multi_device_shares_from_several_host_threads(pkg, dev, monkeypatch):
    """BinMatrix is Send + Sync: several host threads issue products that are each divided among device shares (worker threads,
    leased streams, per-share buffers) at the same time."""
    import threading
    L = pkg._lib.lib()
    nvis = dev.device_count()
    monkeypatch.setenv("M4RI_HIP_DEVICES", ",".join(str(i % nvis) for i in range(3)))
    cases = []
    for k, (m, l, n) in enumerate([(3100, 2050, 1030), (4096, 1024, 2048), (2500, 300, 5000)]):
        a, b = g.random_words(m, l, 50 + k), g.random_words(l, n, 60 + k)
        cases.append((pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n), g.o_mul_m4rm(a, b, m, l, n)))
    bad = []

    def worker(k):
        for it in range(4):
            A, B, ref = cases[(k + it) % len(cases)]
            c = (L.mzd_mul, L.mzd_mul_m4rm)[it & 1](None, A.mzd, B.mzd, 0)
            if not c or not np.array_equal(pkg.BinMatrix(c).to_words(), ref):
                bad.append((k, it))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t_ in ts:
        t_.start()
    for t_ in ts:
        t_.join()
    assert not bad, bad


def test_multi_device_pipelined_shares(pkg, dev):
    """Shares large enough for the per-device upload / compute / download pipeline (>= 16384 rows each)."""
    import ctypes
    L = pkg._lib.lib()
    m, l, n = 32768, 16384, 16384
    a, b = g.random_words(m, l, 44), g.random_words(l, n, 45)
    A, B = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n)
    nvis = dev.device_count()
    arr = (ctypes.c_int * 2)(0, 1 % nvis)
    c = L.gf2_mul_multi(None, A.mzd, B.mzd, dev.ALGO_AUTO, 0, arr, 2)
    assert c
    got = pkg.BinMatrix(c).to_words()
    rows = [0, 1, 16383, 16384, 20000, 32767]
    assert np.array_equal(got[rows], g.o_mul_m4rm(np.ascontiguousarray(a[rows]), b, len(rows), l, n))
    single = L.mzd_mul_m4rm(None, A.mzd, B.mzd, 0)
    assert np.array_equal(got, pkg.BinMatrix(single).to_words())


# ---- size dispatch of the drop-in entry points ---------------------------------------

def test_size_dispatch_of_tiny_products(pkg, monkeypatch):
    """With the default threshold the reference's bench shapes (benches/binary_matrix.rs:30-76) are computed by the
    library's host routines (no PCIe round trip), larger products and everything under M4RI_HIP_HOST_SMALL_WORK=0 (what
    this suite runs with) by the HIP kernels; the bits are the same either way and equal the golden vectors."""
    L = pkg._lib.lib()
    shapes = sorted(glob.glob(os.path.join(GOLDEN, "bench_*.npz")))
    assert len(shapes) >= 11
    for path in shapes:
        z = np.load(path)
        m, l, n = (int(x) for x in z["dims"])
        A, B = pkg.BinMatrix.from_words(z["a"], l), pkg.BinMatrix.from_words(z["b"], n)
        for fn in (lambda: L.mzd_mul(None, A.mzd, B.mzd, 0), lambda: L.mzd_mul_m4rm(None, A.mzd, B.mzd, 0),
                   lambda: L.mzd_mul_naive(None, A.mzd, B.mzd)):
            monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", "0")
            before = L.gf2_host_small_calls()
            dev_c = pkg.BinMatrix(fn()).to_words()
            assert L.gf2_host_small_calls() == before, "the device path was asked for"
            monkeypatch.delenv("M4RI_HIP_HOST_SMALL_WORK")
            host_c = pkg.BinMatrix(fn()).to_words()
            assert L.gf2_host_small_calls() == before + 1, "default threshold: host routine"
            assert np.array_equal(dev_c, z["c"]) and np.array_equal(host_c, z["c"]), os.path.basename(path)
    # above the threshold nothing changes; rank of a tiny matrix takes the host elimination
    monkeypatch.delenv("M4RI_HIP_HOST_SMALL_WORK", raising=False)
    a, b = g.random_words(2048, 2048, 1), g.random_words(2048, 2048, 2)
    before = L.gf2_host_small_calls()
    Abig, Bbig = pkg.BinMatrix.from_words(a, 2048), pkg.BinMatrix.from_words(b, 2048)  # (kept alive across the call)
    c = pkg.BinMatrix(L.mzd_mul(None, Abig.mzd, Bbig.mzd, 0)).to_words()
    assert L.gf2_host_small_calls() == before and np.array_equal(c, g.o_mul_m4rm(a, b, 2048, 2048, 2048))
    low = g.o_mul_naive(g.random_words(40, 7, 3), g.random_words(7, 50, 4), 40, 7, 50)
    assert pkg.BinMatrix.from_words(low, 50).rank() == g.o_echelonize(low, 40, 50)[1] and L.gf2_host_small_calls() == before + 1
    # an operand the caller cached on the device keeps its products there
    A = pkg.BinMatrix.from_words(g.random_words(100, 64, 5), 64)
    assert L.gf2_mzd_cache_on_device(A.mzd) == 0
    before = L.gf2_host_small_calls()
    Bm = pkg.BinMatrix.from_words(g.random_words(64, 10, 6), 10)
    c = pkg.BinMatrix(L.mzd_mul(None, A.mzd, Bm.mzd, 0)).to_words()
    assert L.gf2_host_small_calls() == before
    assert np.array_equal(c, g.o_mul_naive(A.to_words(), Bm.to_words(), 100, 64, 10))
    L.gf2_mzd_uncache(A.mzd)
    monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", "0")


# ---- re-entrancy: BinMatrix is Send + Sync (binary_matrix.rs:38-39) -------------------------------

def test_concurrent_host_threads(pkg):
    """Several host threads multiply shared inputs at once through the C ABI (ctypes drops the GIL)."""
    import threading
    shapes = [(300, 500, 700), (1025, 2049, 513), (64, 4096, 64), (2048, 2048, 2048)]
    mats = []
    for (m, l, n) in shapes:
        a, b = g.random_words(m, l, 31), g.random_words(l, n, 32)
        mats.append((pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n), g.o_mul_m4rm(a, b, m, l, n)))
    L = pkg._lib.lib()
    errors = []

    def worker(k):
        try:
            for it in range(6):
                A, B, ref = mats[(k + it) % len(mats)]
                fn = (L.mzd_mul, L.mzd_mul_m4rm)[it & 1]
                c = fn(None, A.mzd, B.mzd, 0)
                assert c, "NULL product"
                out = pkg.BinMatrix(c)
                if not np.array_equal(out.to_words(), ref):
                    errors.append((k, it))
        except Exception as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_degenerate_shapes(pkg, dev):
    """Empty inner dimension gives the zero matrix; one-row / one-column products; C == A aliasing is not used."""
    L = pkg._lib.lib()
    # l = 0 through the device API (mzd_init allows 0 columns)
    A0, B0 = dev.DMat(5, 0), dev.DMat(0, 70)
    C = dev.DMat.random(5, 70, 9)
    dev.mul(A0, B0, C=C, algo="m4rm")
    assert not dev.DMat.to_words(C).any()
    for (m, l, n) in [(1, 1, 1), (1, 64, 1), (1, 5000, 1), (2, 3, 100000 // 8)]:
        a, b = g.random_words(m, l, 3), g.random_words(l, n, 4)
        ref = g.o_mul_m4rm(a, b, m, l, n)
        for strat in ("strassen", "m4rm", "naive"):
            assert np.array_equal(_host_mul(pkg, a, b, m, l, n, strat), ref), (m, l, n, strat)


def test_split_k_and_small_tile_paths(dev):
    """Shapes that exercise split-K (few tiles, long inner dimension) and the 256-row tile kernel."""
    for (m, l, n) in [(2048, 16384, 2048), (200, 9000, 3000), (1100, 20000, 100), (256, 32768, 4096)]:
        a, b = g.random_words(m, l, 5), g.random_words(l, n, 6)
        ref = g.o_mul_fast(a, b, m, l, n) if (m % 128 == 0 and l % 128 == 0 and n % 128 == 0) else g.o_mul_m4rm(a, b, m, l, n, k=8)
        A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
        assert np.array_equal(dev.mul(A, B, algo="m4rm").to_words(), ref), (m, l, n)
        C0 = dev.DMat.random(m, n, 7)
        c0 = C0.to_words()
        dev.mul(A, B, C=C0, accumulate=True, algo="m4rm")
        assert np.array_equal(C0.to_words(), c0 ^ ref), (m, l, n, "accumulate")


def _tile_plan(dev, m, l, n, batch, packed):
    import ctypes
    plan = (ctypes.c_longlong * 9)()
    dev._lib.lib().gf2_tile_plan(m, l, n, batch, int(packed), plan)
    return list(plan)


def test_streamk_cut_of_the_last_round(dev):
    """Launches whose tiles are a few more than a multiple of 256 (brilliantrussian.rs:210-216 on shapes with 258-276 tiles): the
    whole rounds run whole tiles, the tiles of the last round are cut into stream-K segments whose partial tiles a second kernel
    folds into C -- both kinds of workgroup in ONE launch.  The planner's choice is read back (at least one case must really be
    such a launch), the product is compared with the oracle: whole matrix for the small case, sampled rows otherwise; accumulate
    form too (the reduction kernel then XORs into C)."""
    mixed = 0
    for (m, l, n) in [(4096, 2048, 16896), (8192, 512, 66048), (4096, 2048, 70000), (8192, 2048, 35000)]:
        for packed in (0, 1):
            cfg, _, n_rem, nseg = _tile_plan(dev, m, l, n, 1, packed)[:4]
            if cfg in (9, 10, 11, 12):
                tiles = -(-m // {9: 4096, 10: 2048, 11: 1024, 12: 512}[cfg]) * -(-n // 512)
                mixed += 0 < n_rem < tiles
        a, b = g.random_words(m, l, 21), g.random_words(l, n, 22)
        A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
        rows = np.arange(m) if m * n <= 4096 * 16896 else np.unique(np.concatenate([np.arange(0, m, 509), [m - 1, m // 2, 4095, 4096 % m]]))
        ref = g.o_mul_m4rm(np.ascontiguousarray(a[rows]), b, len(rows), l, n, k=8)
        got = dev.mul(A, B, algo="m4rm").to_words()
        assert np.array_equal(got[rows], ref), (m, l, n)
        C0 = dev.DMat.random(m, n, 23)
        c0 = C0.to_words()
        dev.mul(A, B, C=C0, accumulate=True, algo="m4rm")
        assert np.array_equal(C0.to_words(), c0 ^ got), (m, l, n, "accumulate")
    assert mixed >= 2, "no launch with whole tiles AND segments among the cases: the planner has changed, pick new shapes"


def test_batched_leaves_with_a_tail_launch(dev):
    """A Strassen product whose leaf batch is cut in two launches (strassen.rs:8-18 at 16384^3 with two levels: 49 leaves of 4096^3
    = 392 tiles; the products of the incomplete second round run in a launch of their own with shorter tiles cut into segments):
    same bits as plain M4RM on the device and as the oracle on sampled rows."""
    n = 16384
    plan = _tile_plan(dev, 4096, 4096, 4096, 49, 1)
    assert plan[5] > 0 and plan[6] in (9, 10, 11, 12), ("the planner no longer cuts this batch: pick another shape", plan)
    A, B = dev.DMat.random(n, n, 31), dev.DMat.random(n, n, 32)
    P2 = dev.mul(A, B, algo="strassen", param=2)
    assert dev.equal(P2, dev.mul(A, B, algo="m4rm"))
    rows = [0, 4095, 4096, 9999, n - 1]
    a = np.ascontiguousarray(g.random_words(n, n, 31)[rows])
    assert np.array_equal(P2.to_words()[rows], g.o_mul_m4rm(a, g.random_words(n, n, 32), len(rows), n, n, k=8))
    C0 = dev.DMat.random(n, n, 33)
    expect = dev.add(C0, P2)
    dev.mul(A, B, C=C0, accumulate=True, algo="strassen", param=2)
    assert dev.equal(C0, expect)


def _tile_plan_band(dev, m, l, n, batch, packed):
    import ctypes
    band = (ctypes.c_longlong * 5)()
    dev._lib.lib().gf2_tile_plan_band(m, l, n, batch, int(packed), band)
    return list(band)


def test_row_band_launches(dev):
    """Row counts a little above a multiple of the tile height (brilliantrussian.rs:210-216 on 8512, 8600 and 12700 rows): the
    whole tile rows run as one launch, the rows below them as a second launch with shorter tiles -- disjoint rows of A and C, the
    same B.  The planner's choice is read back (the cases must really have a band); every row of the band and sampled rows above it
    are compared with the oracle, and the accumulate form with the plain sum."""
    banded = 0
    for (m, l, n) in [(8512, 1024, 32768), (8600, 2048, 66000), (12700, 1024, 40000)]:
        rows_band = max(_tile_plan_band(dev, m, l, n, 1, p)[0] for p in (0, 1))
        banded += rows_band > 0
        a, b = g.random_words(m, l, 41), g.random_words(l, n, 42)
        A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
        rows = np.unique(np.concatenate([np.arange(0, m, 997), np.arange(m - max(rows_band, 64) - 2, m), [4095, 4096, 8191, 8192]]))
        ref = g.o_mul_m4rm(np.ascontiguousarray(a[rows]), b, len(rows), l, n, k=8)
        got = dev.mul(A, B, algo="m4rm").to_words()
        assert np.array_equal(got[rows], ref), (m, l, n)
        C0 = dev.DMat.random(m, n, 43)
        c0 = C0.to_words()
        dev.mul(A, B, C=C0, accumulate=True, algo="m4rm")
        assert np.array_equal(C0.to_words(), c0 ^ got), (m, l, n, "accumulate")
    assert banded == 3, "a case lost its row band: the planner has changed, pick new shapes"


def test_batched_leaves_with_a_row_band(dev):
    """Strassen leaves with 4288 rows (strassen.rs:8-18 at 17152 x 4096 x 8192, two levels: 49 packed leaves of 4288 x 1024 x 2048):
    one tile row of 4096 per leaf in the main launch, the 192 rows below it in a band launch over the same batch."""
    m, l, n = 17152, 4096, 8192
    band = _tile_plan_band(dev, m >> 2, l >> 2, n >> 2, 49, 1)
    assert band[0] > 0 and band[1] in (9, 10, 11, 12), ("the planner no longer cuts a band off these leaves: pick another shape", band)
    A, B = dev.DMat.random(m, l, 51), dev.DMat.random(l, n, 52)
    P2 = dev.mul(A, B, algo="strassen", param=2)
    assert dev.equal(P2, dev.mul(A, B, algo="m4rm"))
    rows = np.unique(np.concatenate([np.arange(0, m, 1531), np.arange(4096, 4288), np.arange(m - 192, m)]))
    a = np.ascontiguousarray(g.random_words(m, l, 51)[rows])
    assert np.array_equal(P2.to_words()[rows], g.o_mul_m4rm(a, g.random_words(l, n, 52), len(rows), l, n, k=8))
    C0 = dev.DMat.random(m, n, 53)
    expect = dev.add(C0, P2)
    dev.mul(A, B, C=C0, accumulate=True, algo="strassen", param=2)
    assert dev.equal(C0, expect)


def test_dev_full_size_65536(dev):
    """BASELINE's metric size on one GPU: Strassen (4 fused levels) over M4RM == plain M4RM == oracle on sampled rows."""
    n = 65536
    A, B = dev.DMat.random(n, n, 1), dev.DMat.random(n, n, 2)
    P_auto = dev.mul(A, B)
    P_m4rm = dev.mul(A, B, algo="m4rm")
    assert dev.equal(P_auto, P_m4rm)
    del P_m4rm
    # rows of C from the oracle's vector-matrix product: c_i = a_i * B (reads all of B, cheap for a few rows)
    rows = [0, 12345, 65535]
    w = n // 64
    b = g.random_words(n, n, 2)
    t = np.arange(w, dtype=np.uint64)
    c = P_auto.to_words()
    for r in rows:
        a_r = g.splitmix64(1, np.uint64(r * w) + t).reshape(1, w)
        ref = g.o_mul_m4rm(np.ascontiguousarray(a_r), b, 1, n, n)
        assert np.array_equal(c[r:r + 1], ref), r


def test_host_transpose_large_uses_device_and_matches(pkg):
    """mzd_transpose on big host matrices goes through the device kernel; same bits as the oracle / host routine."""
    for (r, c) in [(4096, 4100), (5000, 4096), (8192, 8192)]:
        w = g.random_words(r, c, 41)
        m = pkg.BinMatrix.from_words(w, c)
        t = m.transposed()
        assert t.nrows() == c and t.ncols() == r
        assert np.array_equal(t.to_words(), g.o_transpose(w, r, c)), (r, c)
        assert t.transposed() == m


@pytest.mark.parametrize("r,c", [(32768, 65600), (65536, 32800)])
def test_host_transpose_pipelined(pkg, r, c):
    """mzd_transpose on host matrices from 2^31 bits on (at least 32768 rows, a multiple of 512 per block): four (eight from 65536 rows
    on) row blocks of the source go up, are transposed into their words of every destination row and come down through 2-D copies while
    the next block goes up.  Ragged column count; the oracle's bits on every row, and the involution (whose source does not qualify:
    the unpipelined path)."""
    w = g.random_words(r, c, 43)
    m = pkg.BinMatrix.from_words(w, c)
    t = m.transposed()
    assert t.nrows() == c and t.ncols() == r
    assert np.array_equal(t.to_words(), g.o_transpose(w, r, c))
    assert t.transposed() == m


@pytest.mark.parametrize("m,l,n", [(2048, 256, 64), (2048, 256, 65), (2500, 256, 128), (3000, 256, 256), (5000, 100, 1),
                                   (4097, 300, 200), (2049, 1000, 129), (9000, 64, 255), (2300, 129, 130), (70000, 256, 37),
                                   (2048, 8, 256), (6000, 513, 64), (5000, 200, 192), (4100, 193, 100), (8197, 256, 255), (65536, 256, 128),
                                   (4096, 255, 256), (12289, 192, 129), (66000, 256, 256), (65536, 250, 200), (73729, 256, 129)])
def test_tall_skinny_shapes(pkg, dev, m, l, n):
    """n <= 256 with many rows (batches of LPN-style products): both tall-skinny kernels (one lane per row for entries
    up to 16 bytes, one quad per row above), all entry widths, ragged everything, with and without accumulation."""
    a, b = g.random_words(m, l, 300 + n), g.random_words(l, n, 301 + l)
    A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
    ref = g.o_mul_m4rm(a, b, m, l, n)
    C = dev.mul(A, B, algo="m4rm")
    assert np.array_equal(C.to_words(), ref)
    c0 = g.random_words(m, n, 302)
    C = dev.DMat.from_words(c0, n)
    dev.mul(A, B, C, accumulate=True, algo="auto")
    assert np.array_equal(C.to_words(), ref ^ c0)


def _strided(dev, words, ncols, ld, offset_words=0):
    """A device matrix holding `words` with row stride `ld` (caller-owned torch memory), optionally starting `offset_words` into it."""
    import torch
    m, w = words.shape
    t = torch.zeros(m * ld + offset_words + 8, dtype=torch.int64, device="cuda")
    v = t[offset_words:offset_words + m * ld].view(m, ld)
    v[:, :w] = torch.from_numpy(words.view(np.int64)).cuda()
    return dev.DMat.wrap(t.data_ptr() + 8 * offset_words, m, ncols, ld, keep=t)


@pytest.mark.parametrize("m,l,n", [(300001, 256, 64), (300001, 256, 100), (300001, 256, 256), (600007, 256, 129), (600007, 256, 200),
                                   (270000, 200, 192), (270000, 192, 256), (2048, 256, 256), (131072, 256, 37), (1048577, 256, 7 * 8 + 9)])
def test_lpn_kernels_rows_per_workgroup(dev, m, l, n):
    """The single-phase l <= 256 kernels (gf2_lpn8_kernel / gf2_lpn256_kernel; mzd_mul_naive as mul_slice reaches it,
    binary_matrix.rs:416-431) choose the rows of a workgroup by the row count: 2048 ... 2^20 + 1 rows cover 1, 2, 4 and 8 row steps
    per lane, a ragged last wave (wave-contiguous loads clamp their addresses, the swapped stores are guarded per row), every entry
    width (64 / 128 / 129-192 / 256 columns); the oracle's bits, overwrite and accumulate."""
    a, b = g.random_words(m, l, 900 + n), g.random_words(l, n, 901 + l)
    A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
    ref = g.o_mul_m4rm(a, b, m, l, n)
    assert np.array_equal(dev.mul(A, B, algo="naive").to_words(), ref)
    c0 = g.random_words(m, n, 902)
    C = dev.DMat.from_words(c0, n)
    dev.mul(A, B, C, accumulate=True, algo="m4rm")
    assert np.array_equal(C.to_words(), ref ^ c0)


@pytest.mark.parametrize("n", [1 * 64, 100, 128, 150, 256])
@pytest.mark.parametrize("lda,ldc_extra,off", [(4, 0, 0), (6, 2, 0), (5, 1, 0), (4, 0, 1), (8, 4, 2)])
def test_lpn_kernels_strides_and_alignment(dev, n, lda, ldc_extra, off):
    """The three load / store forms of the l <= 256 kernels: contiguous A (wave-contiguous 16-byte loads and lane swaps), an even
    row stride (16-byte loads per row), an odd stride or a base that is not 16-byte aligned (8-byte loads); C with its natural stride
    (wave-contiguous 16-byte stores at 256 columns), a wider even one, an odd one.  l = 256 and l = 250 (the last word masked)."""
    m = 70001
    for l in (256, 250):
        a, b = g.random_words(m, l, 950 + n + lda), g.random_words(l, n, 951 + off)
        ref = g.o_mul_m4rm(a, b, m, l, n)
        A = _strided(dev, a, l, lda, off)
        B = dev.DMat.from_words(b, n)
        wn = (n + 63) // 64
        ldc = wn + ldc_extra
        c0 = g.random_words(m, n, 952)
        for acc in (False, True):
            C = _strided(dev, c0, n, ldc, off)
            dev.mul(A, B, C, accumulate=acc, algo="naive")
            assert np.array_equal(C.to_words(), ref ^ c0 if acc else ref), (n, l, lda, ldc, off, acc)


@pytest.mark.parametrize("m,l,n", [(300, 5000, 1), (1000, 70001, 1), (4097, 1500, 8), (2500, 3000, 33), (5000, 2049, 64), (64, 100000, 17),
                                   (16, 600, 3), (2100, 513, 5), (3000, 1025, 9), (777, 8192, 32), (4096, 4096, 2), (150, 200000, 40),
                                   (70000, 1100, 1), (33, 1000000, 4), (70000, 600, 7), (66000, 1000, 50), (140000, 300, 64), (20000, 5000, 12),
                                   (66000, 2049, 10), (1100000, 513, 3), (9000, 33000, 40), (66000, 9000, 20)])
def test_wide_matrix_times_few_vectors(pkg, dev, m, l, n):
    """`&A * &v` and blocks of up to 64 vectors on a matrix with LONG rows (mul_slice, binary_matrix.rs:416-431,528-542, on shapes
    the reference's callers reach with a large square A): the wave-per-row kernel (inner dimension in slabs, 32 vectors per pass)
    and the slab-wise 4-bit table kernel (inner dimension divided among workgroups, atomic XOR into C), ragged everything;
    every algorithm selector gives the oracle's bits, with and without accumulation."""
    a, b = g.random_words(m, l, 500 + n), g.random_words(l, n, 501 + (l % 97))
    A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
    ref = g.o_mul_m4rm(a, b, m, l, n, k=8)
    for algo in ("naive", "auto", "m4rm"):
        assert np.array_equal(dev.mul(A, B, algo=algo).to_words(), ref), (m, l, n, algo)
    c0 = g.random_words(m, n, 502)
    for algo in ("naive", "m4rm"):
        C = dev.DMat.from_words(c0, n)
        dev.mul(A, B, C, accumulate=True, algo=algo)
        assert np.array_equal(C.to_words(), ref ^ c0), (m, l, n, algo, "accumulate")
    # the pre-transposed entry (_mzd_mul_naive, mzd.rs:154-168) reads the vectors as the rows of Bt
    Bt = dev.transpose(B)
    assert np.array_equal(dev.mul_nt(A, Bt).to_words(), ref), (m, l, n, "nt")
    C = dev.DMat.from_words(c0, n)
    dev.mul_nt(A, Bt, C, accumulate=True)
    assert np.array_equal(C.to_words(), ref ^ c0), (m, l, n, "nt accumulate")
    if m <= 70000:  # an odd row stride (caller-owned memory): the 16-byte loads of the fast paths do not apply
        import torch
        wl = (l + 63) // 64
        t = torch.zeros((m, wl + 1 + (wl & 1)), dtype=torch.int64, device="cuda")
        t[:, :wl] = torch.from_numpy(a.view(np.int64)).cuda()
        Aodd = dev.DMat.wrap(t.data_ptr(), m, l, t.shape[1], keep=t)
        assert np.array_equal(dev.mul(Aodd, B, algo="auto").to_words(), ref), (m, l, n, "odd row stride")
    if n == 1 and m * l <= 1 << 27:  # the friendly layer's matrix x vector on host matrices
        M = pkg.BinMatrix.from_words(a, l)
        v = pkg.BinVector.from_bools([bool(int(b[i, 0]) & 1) for i in range(l)])
        assert (M * v).to_bools() == [bool(int(ref[i, 0]) & 1) for i in range(m)]


@pytest.mark.parametrize("m,l,n", [(9, 4096, 16384), (64, 70000, 1024), (33, 40001, 2050), (17, 66000, 4099), (64, 4096, 16385),
                                   (16, 200000, 600), (128, 150001, 100), (100, 20000, 300), (65, 33000, 700), (127, 16384, 65),
                                   (33, 40065, 2050), (17, 66100, 4099)])  # (the last two: l in an odd count of words, Bt has a pad word)
def test_few_rows_times_a_big_matrix(dev, m, l, n):
    """9 to 64 rows against a big B (a block of row vectors times a matrix, brilliantrussian.rs:210-216 with a short A): computed
    transposed, C^T = B^T A^T, through the slab-wise table kernel; the oracle's bits, accumulate form too."""
    a, b = g.random_words(m, l, 700 + m), g.random_words(l, n, 701)
    A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
    ref = g.o_mul_m4rm(a, b, m, l, n, k=8)
    for algo in ("m4rm", "auto"):
        assert np.array_equal(dev.mul(A, B, algo=algo).to_words(), ref), (m, l, n, algo)
    c0 = g.random_words(m, n, 702)
    C = dev.DMat.from_words(c0, n)
    dev.mul(A, B, C, accumulate=True, algo="m4rm")
    assert np.array_equal(C.to_words(), c0 ^ ref), (m, l, n, "accumulate")


@pytest.mark.parametrize("m,l,n", [(3000, 9000, 100), (5000, 8192, 128), (300, 40000, 200), (2049, 33000, 256), (70000, 8200, 65), (1000, 70000, 129),
                                   (4100, 33000, 200), (5000, 40000, 256), (4096, 32768, 193)])
def test_narrow_products_with_long_rows_in_passes(dev, m, l, n):
    """65-256 columns against a long inner dimension (brilliantrussian.rs:210-216 on a narrow B): one pass of the slab-wise table
    kernel per word column where that beats the single column tile of the tile kernel; bits of the oracle, accumulate form too."""
    a, b = g.random_words(m, l, 600 + n), g.random_words(l, n, 601)
    A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
    rows = np.unique(np.concatenate([np.arange(0, m, 37), [m - 1]]))
    ref = g.o_mul_m4rm(np.ascontiguousarray(a[rows]), b, len(rows), l, n, k=8)
    got = dev.mul(A, B, algo="m4rm")
    assert np.array_equal(got.to_words()[rows], ref), (m, l, n)
    assert dev.equal(got, dev.mul(A, B, algo="auto"))
    c0 = g.random_words(m, n, 602)
    C = dev.DMat.from_words(c0, n)
    dev.mul(A, B, C, accumulate=True, algo="m4rm")
    assert np.array_equal(C.to_words()[rows], c0[rows] ^ ref), (m, l, n, "accumulate")


@pytest.mark.parametrize("m,l,n,levels", [(8192, 8192, 8192, 3), (8192, 8192, 8192, 4), (8192, 8192, 8192, 5), (8192, 8192, 8192, 6),
                                          (4160, 8192, 4096, 5), (4096, 2048, 6144, 4), (1000 * 8, 3072, 1024, 3), (2048, 4096, 2048, 4)])
def test_strassen_level_plans(dev, monkeypatch, m, l, n, levels):
    """Every level plan of the Strassen driver -- three fused levels per pass, a virtual fourth on top at 4 levels, pairs
    (M4RI_HIP_STRASSEN_FUSE3=0, round 1's plan) -- gives the bits of plain Four Russians and of the oracle; packed and
    unpacked A leaves (leaf rows a multiple of 64 or not), accumulate form included."""
    A, B = dev.DMat.random(m, l, 11), dev.DMat.random(l, n, 12)
    ref = dev.mul(A, B, algo="m4rm")
    rows = [0, 1, m // 2 - 1, m // 2, m - 1]
    a_rows = np.ascontiguousarray(g.random_words(m, l, 11)[rows])
    assert np.array_equal(ref.to_words()[rows], g.o_mul_m4rm(a_rows, g.random_words(l, n, 12), len(rows), l, n))
    for fuse3 in ("1", "0"):
        monkeypatch.setenv("M4RI_HIP_STRASSEN_FUSE3", fuse3)
        C1 = dev.mul(A, B, algo="strassen", param=levels)
        assert dev.equal(C1, ref), (fuse3, "product")
        C2 = dev.DMat.random(m, n, 13)
        expect = dev.add(C2, ref)
        dev.mul(A, B, C=C2, accumulate=True, algo="strassen", param=levels)
        assert dev.equal(C2, expect), (fuse3, "accumulate")


@pytest.mark.parametrize("m,l,n,levels", [(5000, 4000, 4100, 2), (6000, 6100, 6200, 3), (1030, 2049, 2050, 1), (12000, 12000, 12000, 0),
                                          (8192, 8256, 8192, 0), (4097, 8192, 8192, 4), (8256, 8256, 8256, 2), (16448, 16500, 16390, 0),
                                          (8200, 8192, 8192, 3), (8192, 8192, 8300, 3)])
def test_strassen_on_dimensions_that_do_not_divide(dev, monkeypatch, m, l, n, levels):
    """mzd_mul takes any shape (strassen.rs:8-18; upstream peels): shapes that do not divide by the level plan are padded
    with zeros instead of losing their Strassen levels.  Same bits as plain Four Russians and as the oracle; accumulate
    form; with the padding switched off (M4RI_HIP_STRASSEN_PAD is read once per process, so only the result is compared)."""
    A, B = dev.DMat.random(m, l, 21), dev.DMat.random(l, n, 22)
    ref = dev.mul(A, B, algo="m4rm")
    rows = [0, 1, m // 2, m - 1]
    a_rows = np.ascontiguousarray(g.random_words(m, l, 21)[rows])
    assert np.array_equal(ref.to_words()[rows], g.o_mul_m4rm(a_rows, g.random_words(l, n, 22), len(rows), l, n))
    C1 = dev.mul(A, B, algo="strassen", param=levels)
    assert dev.equal(C1, ref)
    w = C1.to_words()
    if n % 64:
        assert not (w[:, -1] >> np.uint64(n % 64)).any()  # excess bits stay zero
    C2 = dev.DMat.random(m, n, 23)
    expect = dev.add(C2, ref)
    dev.mul(A, B, C=C2, accumulate=True, algo="auto", param=levels)
    assert dev.equal(C2, expect)


@pytest.mark.parametrize("kind", ["sparse", "ones", "zero_a", "identity_b"])
def test_extreme_densities(pkg, dev, kind):
    """Sparse (density 1/64), all-ones and degenerate operands: the table kernels are data-independent, the split-K and
    v*A paths skip zero partial sums; all must agree with the oracle (SURVEY.md section 8d's sanity inputs)."""
    n = 2048
    if kind == "sparse":
        a = g.random_words(n, n, 1)
        b = g.random_words(n, n, 2)
        for k in range(5):
            a &= g.random_words(n, n, 10 + k)
            b &= g.random_words(n, n, 20 + k)
    elif kind == "ones":
        a = np.full((n, n // 64), np.uint64(0xFFFFFFFFFFFFFFFF))
        b = a.copy()
    elif kind == "zero_a":
        a, b = np.zeros((n, n // 64), dtype=np.uint64), g.random_words(n, n, 2)
    else:
        a, b = g.random_words(n, n, 1), g.bits_to_words(np.eye(n, dtype=np.uint8))
    ref = g.o_mul_m4rm(a, b, n, n, n)
    A, B = dev.DMat.from_words(a, n), dev.DMat.from_words(b, n)
    for algo, param in (("m4rm", 0), ("strassen", 1), ("strassen", 2)):
        assert np.array_equal(dev.mul(A, B, algo=algo, param=param).to_words(), ref), (kind, algo, param)


def test_trim_releases_and_work_continues(pkg, dev):
    """gf2_trim gives the scratch arenas and the block cache back to the driver; products afterwards allocate again."""
    import torch
    n = 8192
    A, B = dev.DMat.random(n, n, 1), dev.DMat.random(n, n, 2)
    ref = dev.mul(A, B, algo="m4rm")
    c1 = dev.mul(A, B, algo="strassen", param=3)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    pkg._lib.check(pkg._lib.lib().gf2_trim(), "gf2_trim")
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 >= free0  # at least the Strassen arena went back
    c2 = dev.mul(A, B, algo="strassen", param=3)
    assert dev.equal(c1, ref) and dev.equal(c2, ref)


def test_operand_cache(pkg):
    """gf2_mzd_cache_on_device: a fixed A stays on the device across A*v calls (the LPN use of mul_slice); every library
    call that writes the matrix, and mzd_free, drop the copy."""
    import time
    L = pkg._lib.lib()
    m, l = 1 << 18, 256
    a = g.random_words(m, l, 3)
    A = pkg.BinMatrix.from_words(a, l)
    vs = [pkg.BinVector(g.random_words(1, l, 40 + i)[0], l) for i in range(6)]
    plain = [A * v for v in vs]
    A.cache_on_device()
    cached = [A * v for v in vs]
    assert all(c == p for c, p in zip(cached, plain))
    t0 = time.perf_counter()
    for v in vs:
        A * v
    t_cached = (time.perf_counter() - t0) / len(vs)
    A.uncache()
    t0 = time.perf_counter()
    for v in vs:
        A * v
    t_plain = (time.perf_counter() - t0) / len(vs)
    print("A*v with A (8 MiB) cached: %.0f us, uploaded every call: %.0f us" % (t_cached * 1e6, t_plain * 1e6))
    # writers invalidate: randomize through the library, then the product must see the new bits
    B = pkg.BinMatrix.from_words(g.random_words(300, 200, 5), 200)
    X = pkg.BinMatrix.from_words(g.random_words(200, 100, 6), 100)
    B.cache_on_device()
    first = (B * X).to_words()
    L.mzd_set_ui(B.mzd, 0)  # zero matrix now
    assert not (B * X).to_words().any() and first.any()
    # as a destination
    B.cache_on_device()
    P = pkg.BinMatrix.from_words(g.random_words(300, 50, 7), 50)
    Q = pkg.BinMatrix.from_words(g.random_words(50, 200, 8), 200)
    assert L.mzd_mul(B.mzd, P.mzd, Q.mzd, 0)
    ref = g.o_mul_m4rm(P.to_words(), Q.to_words(), 300, 50, 200)
    assert np.array_equal(B.to_words(), ref)
    assert np.array_equal((B * X).to_words(), g.o_mul_m4rm(ref, X.to_words(), 300, 200, 100))
    # freed and re-created matrices never see a stale copy
    for seed in range(3):
        T = pkg.BinMatrix.from_words(g.random_words(128, 128, 50 + seed), 128)
        T.cache_on_device()
        assert np.array_equal((T * T).to_words(), g.o_mul_m4rm(T.to_words(), T.to_words(), 128, 128, 128))
        del T


@pytest.mark.parametrize("m,n", [(1 << 20, 1), (1 << 18, 3), (300032, 1), (1 << 17, 8), (200001, 2), (300001, 2), (1 << 19, 4), (1 << 19, 5)])
def test_result_side_copy(pkg, m, n):
    """A thin product into a NULL destination comes back with its packed transposed form beside it (m4ri_hip_api.cpp, ResultSide):
    mzd_transpose of that product is served from it and must equal the transposition of the bits the product holds -- for the
    pipelined (A uploaded in row blocks) and the plain (A cached) schedule, ragged row counts included -- and every library call
    that writes the product (mzd_add, mzd_row_swap, a product through a window of it, mzd_copy into it) drops the side copy.
    Stores through rows[] are invisible to the library: INTEGRATION.md 4d says gf2_mzd_uncache after them, checked here too.
    The side copy is opt-in (default off): switched on here with gf2_set_result_side_cols, in this process, so that its kernels (the
    fused product + side launch, the zero-copy route of a pinned A) count in the launch census like every other kernel."""
    L = pkg._lib.lib()
    prev = L.gf2_set_result_side_cols(8)
    try:
        _result_side_copy_opted_in(pkg, L, m, n)
    finally:
        L.gf2_set_result_side_cols(prev)


def _result_side_copy_opted_in(pkg, L, m, n):
    l = 256
    a, x = g.random_words(m, l, 3), g.random_words(l, n, 4)
    A, X = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(x, n)
    ref = g.o_mul_naive(a, x, m, l, n)
    reft = g.o_transpose(ref, m, n)
    for cached in (False, True):
        if cached:
            A.cache_on_device()
        R = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))
        assert np.array_equal(R.to_words(), ref)
        T = R.transposed()  # from the side copy
        assert T.nrows() == n and T.ncols() == m and np.array_equal(T.to_words(), reft)
        T2 = pkg.BinMatrix.zero(n, m)  # a preallocated destination as well
        assert L.mzd_transpose(T2.mzd, R.mzd) and np.array_equal(T2.to_words(), reft)
        # a library write to the product drops the side copy: add another matrix into it
        y = g.random_words(m, n, 9)
        Y = pkg.BinMatrix.from_words(y, n)
        assert L.mzd_add(R.mzd, R.mzd, Y.mzd)
        now = ref ^ y
        assert np.array_equal(R.transposed().to_words(), g.o_transpose(now, m, n))
        # a fresh product again, then a row swap
        R = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))
        i, j = 5, m - 7
        L.mzd_row_swap(R.mzd, i, j)
        sw = ref.copy()
        sw[[i, j]] = sw[[j, i]]
        assert np.array_equal(R.transposed().to_words(), g.o_transpose(sw, m, n))
        # a product THROUGH A WINDOW of a fresh product (rows 64.. of it overwritten)
        R = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))
        rows_w = 4096
        W = L.mzd_init_window(R.mzd, 64, 0, 64 + rows_w, n)
        Aw = pkg.BinMatrix.from_words(a[1000:1000 + rows_w], l)
        assert L.mzd_mul_naive(W, Aw.mzd, X.mzd)
        L.mzd_free(W)
        win = ref.copy()
        win[64:64 + rows_w] = ref[1000:1000 + rows_w]
        assert np.array_equal(R.transposed().to_words(), g.o_transpose(win, m, n))
        # a store through rows[] + gf2_mzd_uncache (what INTEGRATION.md 4d asks of the caller)
        R = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))
        view = R._words_view()
        view[11, 0] ^= np.uint64(1)
        L.gf2_mzd_uncache(R.mzd)
        st = ref.copy()
        st[11, 0] ^= np.uint64(1)
        assert np.array_equal(R.transposed().to_words(), g.o_transpose(st, m, n))
    A.uncache()
    # the reference's operator end to end (binary_matrix.rs:528-542) on the first column
    if n == 1:
        v = pkg.BinVector(g.random_words(1, l, 4)[0], l)
        xv = g.o_transpose(g.random_words(1, l, 4), 1, l)
        got = A * v
        want = g.o_transpose(g.o_mul_naive(a, xv, m, l, 1), m, 1)[0]
        assert len(got) == m and np.array_equal(np.asarray(got.get_storage(), dtype=np.uint64), want)


def test_pinned_pool_keeps_row_pointers(pkg):
    """A pooled pinned block keeps its row-pointer array (mzd_host.cpp): the next matrix of the same shape takes both, a matrix of
    another shape with the same byte count gets a fresh array -- rows[i] must be right either way."""
    L = pkg._lib.lib()
    import ctypes
    for (r, c) in [(1 << 18, 1), (1 << 17, 100), (1 << 18, 64), (1 << 16, 256), (1 << 18, 1)]:
        M = L.mzd_init(r, c)
        mz = M.contents
        stride = mz.rowstride
        base = ctypes.cast(mz.rows[0], ctypes.c_void_p).value
        for i in (0, 1, r // 2, r - 1):
            assert ctypes.cast(mz.rows[i], ctypes.c_void_p).value == base + 8 * stride * i, (r, c, i)
        assert not mz.rows[r]
        L.mzd_free(M)


def test_random_shape_fuzz(pkg):
    """tools/fuzz_shapes.py: log-uniform random shapes (incl. tall-skinny ones) through three algorithms and the
    elimination, all against the oracle."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_shapes.py"), "80", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 40, 100, 200])
@pytest.mark.parametrize("m,mode", [(1048576, 0), (1048576, 1), (1048576, 2), (600001, 0), (600001, 1), (600001, 2), (300003, 0), (300003, 1), (300003, 2)])
def test_lpn_kernels_every_instantiation(dev, m, mode, n):
    """Every (rows per lane, loader) instantiation of the l <= 256 kernels that the launcher can choose (tools/kernel_coverage.py found 20
    of them never launched by this suite): rows per lane 8 / 4 / 2 / 1 by the row count, loader 2 = contiguous 256-bit rows, 1 = strided
    16-byte-aligned rows, 0 = any stride / l <= 192.  n <= 4: the table-free kernel for one to four vectors (gf2_lpnvec_kernel)."""
    l = 256 if mode else 190
    a, b = g.random_words(m, l, 40 + n), g.random_words(l, n, 41 + n)
    ref = g.o_mul_m4rm(a, b, m, l, n)
    B = dev.DMat.from_words(b, n)
    A = dev.DMat.from_words(a, l) if mode != 1 else _strided(dev, a, l, 6)
    C = dev.mul(A, B, algo="naive")
    assert np.array_equal(C.to_words(), ref)
    dev.mul(A, B, C=C, accumulate=True, algo="m4rm")
    assert not C.to_words().any()


@pytest.mark.parametrize("m,l,n", [(524288, 300, 40), (524365, 1000, 64), (524288, 512, 100), (524300, 1024, 200), (524288, 700, 256),
                                   (600000, 257, 65), (530000, 999, 129)])
def test_table_kernels_long_inner_dimension_many_rows(dev, m, l, n):
    """256 < l <= 1024 with at least 2^19 rows: gf2_tallskinny3_kernel (all of B's tables in LDS, 16- and 32-byte entries) for more
    than 64 columns, the slab table kernel (gf2_tallskinny7_kernel) for up to 64 -- the shipped library no longer carries the
    generation kernel gf2_tallskinny4_kernel those used to take; below 2^19 rows these shapes take the tile kernel, so the suite
    never reached them after the threshold moved (tools/kernel_coverage.py)."""
    a, b = g.random_words(m, l, 50 + n), g.random_words(l, n, 51 + n)
    ref = g.o_mul_m4rm(a, b, m, l, n)
    A, B = dev.DMat.from_words(a, l), dev.DMat.from_words(b, n)
    for algo in ("m4rm", "naive"):
        assert np.array_equal(dev.mul(A, B, algo=algo).to_words(), ref), algo
    c0 = g.random_words(m, n, 52)
    C = dev.DMat.from_words(c0, n)
    dev.mul(A, B, C=C, accumulate=True, algo="m4rm")
    assert np.array_equal(C.to_words(), ref ^ c0)


@pytest.mark.parametrize("l", [1, 50, 64, 65, 128, 200, 256, 500, 512, 513, 1000])
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_mul_nt_every_row_width(dev, l, n):
    """_mzd_mul_naive with the pre-transposed operand (mzd.rs:154-168; gf2_mul_nt_dev): the AND / popcount kernel has one
    instantiation per row width (1, 2, 4, 8 words in registers, longer rows in a loop) -- the one- and two-word ones were never
    launched by the suite (tools/kernel_coverage.py)."""
    m = 3001
    a, b = g.random_words(m, l, 60 + l), g.random_words(l, n, 61 + n)
    A, Bt = dev.DMat.from_words(a, l), dev.DMat.from_words(g.o_transpose(b, l, n), l)
    ref = g.o_mul_naive(a, b, m, l, n)
    assert np.array_equal(dev.mul_nt(A, Bt).to_words(), ref)
    if l > 64:  # unaligned rows: odd stride
        assert np.array_equal(dev.mul_nt(_strided(dev, a, l, (l + 63) // 64 | 1, offset_words=1), Bt).to_words(), ref)


def test_result_side_copy_can_be_switched_off(pkg):
    """M4RI_HIP_RESULT_SIDE_COLS=0 (the default since the side copy became opt-in; set explicitly here): no product carries a side copy, so even a store through rows[] WITHOUT gf2_mzd_uncache is seen by the next
    mzd_transpose -- and the operator still gives the right bits, A uploaded or cached.  In a child process: the variable is read once."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')\n"
              "import numpy as np, gf2util as g, m4ri_rust_amd as pkg\n"
              "L = pkg._lib.lib(); m, l = 1 << 19, 256\n"
              "a, x = g.random_words(m, l, 3), g.random_words(l, 1, 4)\n"
              "A, X = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(x, 1)\n"
              "ref = g.o_mul_naive(a, x, m, l, 1)\n"
              "for cached in (False, True):\n"
              "    if cached: A.cache_on_device()\n"
              "    R = pkg.BinMatrix(L.mzd_mul_naive(None, A.mzd, X.mzd))\n"
              "    assert np.array_equal(R.to_words(), ref)\n"
              "    R._words_view()[11, 0] ^= np.uint64(1)   # a plain store, no gf2_mzd_uncache\n"
              "    st = ref.copy(); st[11, 0] ^= np.uint64(1)\n"
              "    assert np.array_equal(R.transposed().to_words(), g.o_transpose(st, m, 1))\n"
              "print('OK')\n") % (root, root)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, M4RI_HIP_RESULT_SIDE_COLS="0"), timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_lpn_operator_from_several_host_threads(pkg):
    """`BinMatrix: Send + Sync` (binary_matrix.rs:38-39): four host threads run the reference's LPN operator `&A * &v` at once -- one shared
    A (uploaded per call: the zero-copy vector kernel; then cached on the device), every thread its own vectors --, so the side copies,
    the pooled pinned blocks with their row-pointer arrays and the per-thread streams are exercised concurrently; every result is
    checked against the oracle."""
    L = pkg._lib.lib()
    prev = L.gf2_set_result_side_cols(8)  # the side copies opted in, as the docstring says
    try:
        _lpn_operator_threads(pkg)
    finally:
        L.gf2_set_result_side_cols(prev)


def _lpn_operator_threads(pkg):
    import threading
    m, l = 1 << 19, 256
    a = g.random_words(m, l, 3)
    A = pkg.BinMatrix.from_words(a, l)
    nthreads, per = 4, 6
    xs = [[g.random_words(1, l, 100 + 10 * t + i) for i in range(per)] for t in range(nthreads)]
    want = [[g.o_transpose(g.o_mul_naive(a, g.o_transpose(x, 1, l), m, l, 1), m, 1)[0] for x in row] for row in xs]
    for cached in (False, True):
        if cached:
            A.cache_on_device()
        bad = []

        def worker(t):
            for i in range(per):
                got = A * pkg.BinVector(xs[t][i][0], l)
                if len(got) != m or not np.array_equal(np.asarray(got.get_storage(), dtype=np.uint64), want[t][i]):
                    bad.append((t, i))

        ts = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
        for t_ in ts:
            t_.start()
        for t_ in ts:
            t_.join()
        assert not bad, (cached, bad)
    A.uncache()
