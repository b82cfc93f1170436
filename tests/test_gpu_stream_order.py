"""Stream ordering of the device-resident API (include/m4ri_hip.h, section 2) on caller streams.

Every test here makes its library calls on a fresh, non-blocking stream behind about 0.1 s of queued sleep (tests/stream_util.py):
the inputs are written by copies queued behind the sleep into tensors that hold a poison pattern until then, every output tensor
gets such a pending copy of junk too, the results are read by torch ops on the same stream, and nothing synchronises in between.
A launch, a memset or a copy of the library that goes to another stream (or to the host) runs while the stream still sleeps: it reads
poison, or the pending copies overwrite what it wrote.  A scratch arena shared between streams, handed back too early or recycled
under queued work is overwritten while the delayed work uses it.  The sleep makes that window wide: a correct library can never fail
these tests, a wrong one fails them with near certainty and not by luck.  Every comparison is bit for bit against the CPU references
of the suite (gf2util.o_*, trsm_ref, splitmix64), never against another device result.

Entries of section 2 that take a stream, and the tests that call them on a caller's stream behind pending work:
  gf2_mul_dev                      test_mul_dev (every host path, plain and accumulate), the chains, two streams, threads
  gf2_mul_nt_dev                   test_mul_nt_dev
  gf2_add_dev, gf2_transpose_dev   test_add_and_transpose_dev, test_dependent_chain
  gf2_equal_dev                    test_equal_dev
  gf2_dmat_fill_random, _rows, _block   test_fill_random
  gf2_dmat_upload                  test_upload_then_product
  gf2_dmat_download                test_download_of_a_pending_product
  gf2_trsm_dev                     test_trsm_dev, test_trsm_dev_block_64, the chains, two streams, threads
  gf2_apply_p_dev                  test_apply_p_dev
  gf2_echelonize_dev               test_echelonize_dev
  gf2_inverse_dev                  test_inverse_dev
  gf2_dmat_free_async, gf2_dmat_free   test_free_async_keeps_the_block_until_the_stream_has_passed, test_free_waits_for_pending_work,
                                   test_python_temporaries_in_a_chain
  gf2_trim                         test_trim_then_the_streams_rebuild_their_arenas
  gf2_ple_dev, gf2_pluq_solve_left_dev   tests/test_gpu_ple_exact.py (test_ple_on_caller_stream, test_solve_on_caller_stream)
"""
import ctypes
import functools
import threading

import numpy as np
import pytest

import gf2util as g
import trsm_ref as R
from stream_util import lanes, on_stream, padded, run_pending

pytestmark = pytest.mark.gpu

D = 512  # TRSM_BLOCK of gf2_trsm.hip


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


def cut(x, ncols):
    """the valid words of a matrix read back with its (even) row stride"""
    return np.ascontiguousarray(x[:, :g.width(ncols)])


def tile_plan(dev, m, l, n, batch=1, packed=0):
    out = (ctypes.c_longlong * 9)()
    dev._lib.lib().gf2_tile_plan(m, l, n, batch, packed, out)
    return list(out)


def mul_plan(dev, m, l, n, algo, param):
    kind, dims = ctypes.c_int(0), (ctypes.c_int * 3)()
    levels = dev._lib.lib().gf2_mul_plan(m, l, n, dev.ALGOS[algo], param, ctypes.byref(kind), dims)
    return levels, kind.value, list(dims)


def ws_bytes(dev, m, l, n, algo, param=0):
    return dev._lib.lib().gf2_mul_workspace_bytes(m, l, n, dev.ALGOS[algo], param)


def even(w):
    return (w + 1) & ~1


@functools.lru_cache(maxsize=None)
def product(m, l, n, seed):
    """(a, b, c0, a*b) of a seeded product; computed once, shared, never written"""
    a, b, c0 = g.random_words(m, l, seed), g.random_words(l, n, seed + 1), g.random_words(m, n, seed + 2)
    out = (a, b, c0, g.o_mul_fast(a, b, m, l, n))
    for x in out:
        x.setflags(write=False)
    return out


def mul_on_stream(dev, m, l, n, seed, acc, algo, param=0):
    a, b, c0, ref = product(m, l, n, seed)
    srcs = [padded(a), padded(b), padded(c0)]

    def issue(ls):
        t, s = ls[0].live, ls[0].handle
        dev.mul(dev.DMat.from_torch(t[0], l), dev.DMat.from_torch(t[1], n), C=dev.DMat.from_torch(t[2], n), accumulate=bool(acc),
                algo=algo, param=param, stream=s)

    def check(_, outs):
        ga, gb, gc = outs[0]
        assert np.array_equal(ga, srcs[0]) and np.array_equal(gb, srcs[1]), "an operand changed"
        assert np.array_equal(cut(gc, n), ref ^ c0 if acc else ref), (m, l, n, algo, param, "accumulate" if acc else "plain")

    run_pending([srcs], issue, check)


# ---- 1. every entry on a caller's stream behind pending work -------------------------------------------------------------

def plan_streamk(dev, m, l, n):  # stream-K partial tiles: slot 1
    p = tile_plan(dev, m, l, n)
    assert p[0] in (9, 10, 11, 12) and p[2] > 0 and p[4] > 0, ("no stream-K cut any more: pick another shape", p)
    assert ws_bytes(dev, m, l, n, "m4rm") >= p[4]


def plan_packed(dev, m, l, n):  # a packed copy of A (slot 2) next to the partial tiles (slot 1)
    p = tile_plan(dev, m, l, n, 1, 1)
    pack = ((m + 63) & ~63) * even(g.width(l)) * 8
    assert p[2] > 0 and p[4] > 0 and ws_bytes(dev, m, l, n, "m4rm") == p[4] + pack, ("A is no longer packed: pick another shape", p)


def plan_strassen(levels, kind):
    def check(dev, m, l, n):
        got = mul_plan(dev, m, l, n, "strassen", levels)
        assert got[:2] == (levels, kind), ("the planner runs this shape another way: pick another shape", got)
        assert ws_bytes(dev, m, l, n, "strassen", levels) > 0
    return check


def plan_transposed_vectors(dev, m, l, n):  # the wave-per-row kernel: B transposed into slot 0
    for algo in ("naive", "m4rm"):
        assert ws_bytes(dev, m, l, n, algo) == n * even(g.width(l)) * 8, "no longer the wave-per-row path: pick another shape"


def plan_few_rows(dev, m, l, n):  # computed transposed: B^T, A^T, C^T (and a copy of the product when accumulating) in slot 0
    want = (n * even(g.width(l)) + 2 * l + n * even(g.width(m)) + m * even(g.width(n))) * 8
    assert ws_bytes(dev, m, l, n, "m4rm") == want, "no longer the transposed few-rows path: pick another shape"


def plan_tables(dev, m, l, n):  # the LPN table kernels need no scratch
    assert ws_bytes(dev, m, l, n, "m4rm") == 0


MUL_CASES = [
    # tests/test_gpu_views.py ROUTES "v8-streamk": variant 11, 9 tiles cut into segments
    ("streamk", "m4rm", 0, 1000, 1025, 4097, plan_streamk),
    # the smallest shape of test_split_k_and_small_tile_paths (test_gpu_parity.py): at the stream-K shape above A is not packed
    ("streamk-packed-a", "m4rm", 0, 2048, 16384, 2048, plan_packed),
    # test_strassen_packed_leaves (test_gpu_parity.py)
    ("strassen-2", "strassen", 2, 1280, 2048, 1024, plan_strassen(2, 0)),
    # test_strassen_on_dimensions_that_do_not_divide (test_gpu_parity.py): its smallest shape is padded; its only peeled one
    ("strassen-padded", "strassen", 1, 1030, 2049, 2050, plan_strassen(1, 1)),
    ("strassen-peeled", "strassen", 3, 8192, 8192, 8300, plan_strassen(3, 2)),
    # test_wide_matrix_times_few_vectors (test_gpu_parity.py), its smallest shape on the wave-per-row path: through mul_naive_dev ...
    ("naive-transposed-b", "naive", 0, 300, 5000, 1, plan_transposed_vectors),
    # ... and through the plain dispatch
    ("wave-per-row", "m4rm", 0, 300, 5000, 1, plan_transposed_vectors),
    # test_few_rows_times_a_big_matrix (test_gpu_parity.py), its smallest shape that is computed transposed
    ("few-rows", "m4rm", 0, 100, 20000, 300, plan_few_rows),
    # test_tall_skinny_shapes (test_gpu_parity.py)
    ("lpn-tables", "m4rm", 0, 2048, 256, 64, plan_tables),
]


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("case", MUL_CASES, ids=[c[0] for c in MUL_CASES])
def test_mul_dev(dev, case, acc):
    _, algo, param, m, l, n, plan = case
    plan(dev, m, l, n)
    mul_on_stream(dev, m, l, n, 100 + m % 97 + n % 89, acc, algo, param)


# (300, 5000, 1): the wave-per-row branch (test_wide_matrix_times_few_vectors); (3001, 200, 65): the AND / popcount kernel
# (test_mul_nt_every_row_width)
@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("m,l,n", [(300, 5000, 1), (3001, 200, 65)])
def test_mul_nt_dev(dev, m, l, n, acc):
    a, b, c0, ref = product(m, l, n, 7)
    bt = g.o_transpose(b, l, n)
    srcs = [padded(a), padded(bt), padded(c0)]

    def issue(ls):
        t, s = ls[0].live, ls[0].handle
        dev.mul_nt(dev.DMat.from_torch(t[0], l), dev.DMat.from_torch(t[1], l), C=dev.DMat.from_torch(t[2], n), accumulate=bool(acc),
                   stream=s)

    def check(_, outs):
        assert np.array_equal(cut(outs[0][2], n), ref ^ c0 if acc else ref)

    run_pending([srcs], issue, check)


def test_add_and_transpose_dev(dev):
    m, n = 1000, 4097
    a, b = g.random_words(m, n, 1), g.random_words(m, n, 2)
    junk_c, junk_d = g.random_words(m, n, 3), g.random_words(n, m, 4)

    want_t = g.o_transpose(a ^ b, m, n)

    def issue(ls):
        t, s = ls[0].live, ls[0].handle
        C = dev.add(dev.DMat.from_torch(t[0], n), dev.DMat.from_torch(t[1], n), C=dev.DMat.from_torch(t[2], n), stream=s)
        dev.transpose(C, D=dev.DMat.from_torch(t[3], m), stream=s)  # of the sum: depends on the add as well

    def check(_, outs):
        assert np.array_equal(cut(outs[0][2], n), a ^ b)
        assert np.array_equal(cut(outs[0][3], m), want_t)

    run_pending([[padded(a), padded(b), padded(junk_c), padded(junk_d)]], issue, check)


@pytest.mark.parametrize("same", [False, True], ids=["different", "equal"])
def test_equal_dev(dev, same):
    """the answer must come from what the pending copies write: before them the two buffers are equal (both poison) where the
    answer is "different", and different where the answer is "equal\""""
    m, n = 1000, 4097
    a = g.random_words(m, n, 5)
    b = a.copy()
    if not same:
        b[m - 1, g.width(n) - 1] ^= np.uint64(1)  # the last valid bit
    (lane,) = lanes([padded(a), padded(b)])
    if same:
        import torch
        lane.live[1].fill_(0x33)
        torch.cuda.synchronize()
    lane.open()
    got = dev.equal(dev.DMat.from_torch(lane.live[0], n), dev.DMat.from_torch(lane.live[1], n), stream=lane.handle)
    assert got is same


def test_fill_random(dev):
    L = dev._lib.lib()
    m, n, w = 1000, 4097, g.width(4097)
    row0, brow0, bcol0, full = 12345, 77, 5, 9000
    junk = padded(g.random_words(m, n, 6))

    def issue(ls):
        t, s = ls[0].live, ls[0].handle
        M = [dev.DMat.from_torch(x, n) for x in t]
        dev._lib.check(L.gf2_dmat_fill_random(M[0]._on(s), 41, s), "fill_random")
        dev._lib.check(L.gf2_dmat_fill_random_rows(M[1]._on(s), 42, row0, s), "fill_random_rows")
        dev._lib.check(L.gf2_dmat_fill_random_block(M[2]._on(s), 43, brow0, bcol0, full, s), "fill_random_block")

    mask = np.uint64((1 << (n % 64)) - 1)
    i, j = np.indices((m, w), dtype=np.uint64)

    def want(seed, r0, fullw, c0):
        x = g.splitmix64(seed, (i + np.uint64(r0)) * np.uint64(fullw) + np.uint64(c0) + j)
        x[:, -1] &= mask
        return x

    wants = [want(41, 0, w, 0), want(42, row0, w, 0), want(43, brow0, g.width(full), bcol0)]
    assert np.array_equal(wants[0], g.random_words(m, n, 41))

    def check(_, outs):
        for x, ref in zip(outs[0], wants):
            assert np.array_equal(cut(x, n), ref)
            assert np.array_equal(x[:, w:], junk[:, w:]), "words past the row width changed"

    run_pending([[junk, junk, junk]], issue, check)


def test_upload_then_product(pkg, dev):
    """the upload must wait behind the pending copy that writes junk into its destination (on another stream the junk would land
    on top of it); the product then runs behind a second sleep"""
    m, l, n = 1000, 1025, 4097
    a, b, c0, ref = product(m, l, n, 11)
    (lane,) = lanes([padded(g.random_words(m, l, 12)), padded(b), padded(c0)])
    lane.open(only=[0])
    A = dev.DMat.from_torch(lane.live[0], l)
    host = pkg.BinMatrix.from_words(a, l)
    dev._lib.check(dev._lib.lib().gf2_dmat_upload(A._on(lane.handle), host.mzd, lane.handle), "upload")
    lane.open(only=[1, 2])
    dev.mul(A, dev.DMat.from_torch(lane.live[1], n), C=dev.DMat.from_torch(lane.live[2], n), algo="m4rm", stream=lane.handle)
    ga, _, gc = lane.read()
    assert np.array_equal(cut(ga, l), a)
    assert np.array_equal(cut(gc, n), ref)


def test_download_of_a_pending_product(pkg, dev):
    m, l, n = 1000, 1025, 4097
    a, b, c0, ref = product(m, l, n, 11)
    (lane,) = lanes([padded(a), padded(b), padded(c0)])
    lane.open()
    C = dev.mul(dev.DMat.from_torch(lane.live[0], l), dev.DMat.from_torch(lane.live[1], n), C=dev.DMat.from_torch(lane.live[2], n),
                accumulate=True, algo="m4rm", stream=lane.handle)
    host = pkg.BinMatrix.zero(m, n)
    dev._lib.check(dev._lib.lib().gf2_dmat_download(host.mzd, C._on(lane.handle), lane.handle), "download")
    assert np.array_equal(host.to_words(), ref ^ c0)


N_TRSM = 2 * D + 65  # the inversion launch, the recursion's products and the copy-back all occur


@functools.lru_cache(maxsize=None)
def trsm_case(n, k, upper, right, seed):
    """(T bits with anything outside the strict triangle, B0, X by substitution); X is checked through the product as well"""
    rows, cols = R.b_shape(n, k, right)
    tb = R.random_bits(n, n, seed)
    b0 = g.random_words(rows, cols, seed + 1)
    x = R.solve(tb, b0, rows, cols, upper, right)
    R.check_product(tb, x, b0, rows, cols, upper, right)
    for a in (tb, b0, x):
        a.setflags(write=False)
    return tb, b0, x


def trsm_on_stream(dev, n, k, upper, right, seed):
    tb, b0, x = trsm_case(n, k, upper, right, seed)
    cols = R.b_shape(n, k, right)[1]
    tw = padded(g.bits_to_words(tb))

    def issue(ls):
        t, s = ls[0].live, ls[0].handle
        dev.trsm(dev.DMat.from_torch(t[0], n), dev.DMat.from_torch(t[1], cols), upper=upper, right=right, stream=s)

    def check(_, outs):
        assert np.array_equal(outs[0][0], tw), "T changed"
        assert np.array_equal(cut(outs[0][1], cols), x), R.name(upper, right)

    run_pending([[tw, padded(b0)]], issue, check)


@pytest.mark.parametrize("upper,right", R.VARIANTS)
def test_trsm_dev(dev, upper, right):
    trsm_on_stream(dev, N_TRSM, 300 if right else 65, upper, right, 21)


def test_trsm_dev_block_64(dev, monkeypatch):
    monkeypatch.setenv("M4RI_HIP_TRSM_BLOCK", "64")  # 18 diagonal blocks: a deeper recursion, many leaves
    trsm_on_stream(dev, N_TRSM, 300, True, True, 21)


# the second shape of test_apply_p_against_oracle (tests/test_gpu_ple_exact.py)
@pytest.mark.parametrize("right,trans", [(False, False), (False, True), (True, False), (True, True)])
def test_apply_p_dev(dev, right, trans):
    import random
    m, n = 1500, 12000
    a = g.random_words(m, n, 31)
    size = n if right else m
    rng = random.Random(size + trans)
    perm = [rng.randrange(i, size) for i in range(size - 7)]
    _, (got,) = on_stream(dev, [padded(a)], lambda t, s: dev.apply_p(dev.DMat.from_torch(t[0], n), perm, right=right, trans=trans, stream=s))
    assert np.array_equal(cut(got, n), g.o_apply_p(a, m, n, perm, right=right, trans=trans))


def low_rank(m, n, r, seed):
    return g.o_mul_fast(g.random_words(m, r, seed), g.random_words(r, n, seed + 1), m, r, n)


# full: SHAPES of test_rref_random (tests/test_gpu_elim.py): (100, 100) is the one-workgroup path, (513, 1030) the blocked one;
# upper form: test_upper_echelon_form, (100, 100, 100) small and (1500, 1200, 300) blocked
@pytest.mark.parametrize("m,n,r,full", [(100, 100, 100, True), (513, 1030, 513, True), (100, 100, 100, False), (1500, 1200, 300, False)])
def test_echelonize_dev(dev, m, n, r, full):
    a = low_rank(m, n, r, 31) if r < min(m, n) else g.random_words(m, n, 32)
    ref, orank, opiv = g.o_echelonize(a, m, n, full=True)
    (rank, piv), (got,) = on_stream(dev, [padded(a)], lambda t, s: dev.echelonize(dev.DMat.from_torch(t[0], n), full=full, stream=s))
    got = cut(got, n)
    assert rank == orank and piv == opiv
    if full:
        assert np.array_equal(got, ref)
    else:  # as test_upper_echelon_form: echelon shape, the same pivots, the same row space
        bits = g.words_to_bits(got, n)
        assert not bits[rank:].any()
        assert list(np.argmax(bits[:rank], axis=1)) == opiv
        for i, c in enumerate(opiv):
            assert not bits[i + 1:, c].any()
        assert np.array_equal(g.o_echelonize(got, m, n, full=True)[0], ref)


def invertible(n, seed):
    lo = g.bits_to_words(R.clean(R.random_bits(n, n, seed), False))
    up = g.bits_to_words(R.clean(R.random_bits(n, n, seed + 1), True))
    return g.o_mul_fast(lo, up, n, n, n)


@pytest.mark.parametrize("singular", [False, True], ids=["invertible", "singular"])
@pytest.mark.parametrize("n", [200, 1000])
def test_inverse_dev(dev, n, singular):
    a = low_rank(n, n, n - 1, 51) if singular else invertible(n, 52)
    want = g.o_inverse(a, n)
    assert (want is None) == singular
    junk = padded(g.random_words(n, n, 53))

    def call(t, s):
        flag = ctypes.c_int(-1)
        A, Ainv = dev.DMat.from_torch(t[0], n), dev.DMat.from_torch(t[1], n)
        dev._lib.check(dev._lib.lib().gf2_inverse_dev(Ainv._on(s), A._on(s), ctypes.byref(flag), s), "gf2_inverse_dev")
        return flag.value

    flag, (ga, ginv) = on_stream(dev, [padded(a), junk], call)
    assert flag == int(singular)
    assert np.array_equal(cut(ga, n), a), "A changed"
    if singular:
        assert np.array_equal(ginv, junk), "Ainv must stay untouched for a singular matrix"
    else:
        assert np.array_equal(cut(ginv, n), want)


# ---- 2. chains with no host synchronisation in between ------------------------------------------------------------------------

def test_dependent_chain(dev):
    """C1 = A*B, C2 = C1*D, C2 ^= E*F, G = C2^T, G = T^-1 G, H = G ^ W on one stream behind one sleep; the intermediates that a later
    call overwrites are kept by torch copies queued on the stream, and everything is read at the end"""
    m, l, n, q, e = 1000, 1025, 4097, N_TRSM, 300
    a, b, _, c1 = product(m, l, n, 11)
    d, f = g.random_words(n, q, 61), g.random_words(e, q, 62)
    ee, w = g.random_words(m, e, 63), g.random_words(q, m, 64)
    tb = R.random_bits(q, q, 65)
    c2a = g.o_mul_fast(c1, d, m, n, q)
    c2 = c2a ^ g.o_mul_fast(ee, f, m, e, q)
    gt = g.o_transpose(c2, m, q)
    x = R.solve(tb, gt, q, m, False, False)
    R.check_product(tb, x, gt, q, m, False, False)
    junk = [g.random_words(r, c, 66 + i) for i, (r, c) in enumerate(((m, n), (m, q), (q, m), (q, m)))]
    srcs = [padded(v) for v in [a, b, d, ee, f, w, g.bits_to_words(tb)] + junk]

    def issue(ls):
        lane = ls[0]
        t, s = lane.live, lane.handle
        M = dev.DMat.from_torch
        A, B, Dm, E, F, Wm, T = M(t[0], l), M(t[1], n), M(t[2], q), M(t[3], e), M(t[4], q), M(t[5], m), M(t[6], q)
        C1, C2, G, H = M(t[7], n), M(t[8], q), M(t[9], m), M(t[10], m)
        dev.mul(A, B, C=C1, algo="m4rm", stream=s)
        dev.mul(C1, Dm, C=C2, stream=s)
        (first,) = lane.snapshot([t[8]])
        dev.mul(E, F, C=C2, accumulate=True, stream=s)
        dev.transpose(C2, D=G, stream=s)
        (before,) = lane.snapshot([t[9]])
        dev.trsm(T, G, stream=s)
        dev.add(G, Wm, C=H, stream=s)
        return lane, [first, before]

    def check(res, outs):
        lane, kept = res
        got = outs[0]
        gfirst, gbefore = lane.read(kept)
        assert np.array_equal(cut(got[7], n), c1), "C1 = A*B"
        assert np.array_equal(cut(gfirst, q), c2a), "C2 = C1*D"
        assert np.array_equal(cut(got[8], q), c2), "C2 ^= E*F"
        assert np.array_equal(cut(gbefore, m), gt), "G = C2^T"
        assert np.array_equal(cut(got[9], m), x), "G = T^-1 G"
        assert np.array_equal(cut(got[10], m), x ^ w), "H = G ^ W"
        for i in range(7):
            assert np.array_equal(got[i], srcs[i]), ("an input changed", i)

    run_pending([srcs], issue, check)


def free_async(dev, X, stream):
    dev._lib.check(dev._lib.lib().gf2_dmat_free_async(ctypes.byref(X.s), stream), "gf2_dmat_free_async")
    assert not X.s.data


def give_the_pool_a_chance(dev, stream):
    """What a wrong library would hand back too early must be in its pool before the test allocates: work that strayed to the NULL
    stream has finished once that stream is synchronised (this waits for nothing on the caller streams, which are non-blocking),
    and a stream-ordered free of a dummy makes the library look through its deferred frees."""
    import torch
    torch.cuda.default_stream().synchronize()
    free_async(dev, dev.DMat(1, 64), stream)


def junk_writer(dev, lane, nbytes, blocks=4, rounds=48):
    """A second stream that wakes when `lane` does and then keeps filling fresh library blocks of the size class of `nbytes`
    with random words while the lane's delayed work runs: a block that the library handed back too early is among them."""
    import torch
    s2 = torch.cuda.Stream()
    give_the_pool_a_chance(dev, s2.cuda_stream)
    rows = max(1, -(-nbytes // 1024))
    mats = [dev.DMat(rows, 8192) for _ in range(blocks)]  # 1 KiB per row
    s2.wait_event(lane.awake)
    for r in range(rounds):
        for i, X in enumerate(mats):
            X.fill_random(1000 + r * blocks + i, s2.cuda_stream)
    return s2, mats


def trim(dev):
    import torch
    torch.cuda.synchronize()
    dev._lib.check(dev._lib.lib().gf2_trim(), "gf2_trim")


def strassen_arena_bytes(dev, m, l, n, levels):
    """bytes of the operand arena (slot 0): gf2_mul_workspace_bytes less the partial tiles of the leaf launch (slot 1)"""
    leaf = [tile_plan(dev, m >> levels, l >> levels, n >> levels, 7 ** levels, p)[4] for p in (0, 1)]
    assert leaf[0] == leaf[1], "the leaf plans differ in their scratch: pick another shape"
    return ws_bytes(dev, m, l, n, "strassen", levels) - leaf[0]


def test_strassen_arena_grows_under_pending_work(dev):
    """small, large, small in slot 0 of one stream: the second call replaces the arena while the first still has to run (free_after
    in stream_workspace).  The pool is emptied first, so a block that came back too early is the one a new allocation gets."""
    small, big = (1280, 2048, 1024), (2560, 4096, 2048)  # (the first: test_strassen_packed_leaves)
    assert ws_bytes(dev, *big, "strassen", 2) > ws_bytes(dev, *small, "strassen", 2)
    arena = strassen_arena_bytes(dev, *small, 2)
    assert strassen_arena_bytes(dev, *big, 2) > arena + arena // 4 + (1 << 20), "the second arena must not fit into the first block"
    for shape in (small, big):
        assert mul_plan(dev, *shape, "strassen", 2)[:2] == (2, 0)
    p1, p2, p3 = product(*small, 71), product(*big, 72), product(*small, 73)

    def issue(ls):
        lane = ls[0]
        for i, shape in enumerate((small, big, small)):
            A, B, C = (dev.DMat.from_torch(lane.live[3 * i + j], c) for j, c in enumerate((shape[1], shape[2], shape[2])))
            dev.mul(A, B, C=C, accumulate=(i == 2), algo="strassen", param=2, stream=lane.handle)
        return junk_writer(dev, lane, arena)

    def check(_, outs):
        got = outs[0]
        assert np.array_equal(cut(got[2], small[2]), p1[3]), "the product whose arena was replaced under it"
        assert np.array_equal(cut(got[5], big[2]), p2[3])
        assert np.array_equal(cut(got[8], small[2]), p3[3] ^ p3[2])

    trim(dev)
    run_pending([[padded(x) for p in (p1, p2, p3) for x in p[:3]]], issue, check)


def plain_slots(dev, m, l, n):
    """(bytes of partial tiles in slot 1, bytes of the packed A in slot 2) of a plain product, from the planner"""
    total, packed_scratch = ws_bytes(dev, m, l, n, "m4rm"), tile_plan(dev, m, l, n, 1, 1)[4]
    pack = ((m + 63) & ~63) * even(g.width(l)) * 8
    return (packed_scratch, pack) if total == packed_scratch + pack else (total, 0)


def test_trsm_arena_grows_under_pending_work(dev):
    """A small solve, then a larger one on the same stream: both trsm slots outgrow their arenas while the first solve still has
    to run (the block inverses with n; the leaf result of a right-hand variant takes 64 bytes per row of B, so 24000 rows move
    slot 5 out of the 1 MiB block it started in).  A product with a packed A and stream-K scratch goes first: it needs more of
    slots 1 and 2 than any product inside the solves, so no other slot of the stream grows meanwhile and takes the block that
    slot 5 gave up (which would be harmless, and would hide it from the stream that writes junk).
    This pins the results of the sequence.  A block handed back too early is caught with near certainty by the Strassen test above
    and by the address checks of the free tests below, not here: slot 5 holds a leaf result for microseconds only, and the block
    that slot 4 gives up is of the pool's 1 MiB class like its successor, so it returns to the same stream."""
    first = (2048, 16384, 2048)  # "streamk-packed-a" of MUL_CASES
    cases = [trsm_case(n, k, False, True, 81 + n) for n, k in ((D + 65, 300), (N_TRSM, 24000))]
    pk = product(*first, 112)
    have = plain_slots(dev, *first)
    for k in (300, 24000):
        for inner in ((k, D, D), (k, 65, 65), (k, D, 65), (k, 2 * D, 65)):  # leaves and updates of the recursion
            need = plain_slots(dev, *inner)
            assert need[0] <= have[0] and need[1] <= have[1], ("a product inside the solves outgrows the first product", inner, need, have)

    def issue(ls):
        lane = ls[0]
        M = dev.DMat.from_torch
        dev.mul(M(lane.live[0], first[1]), M(lane.live[1], first[2]), C=M(lane.live[2], first[2]), algo="m4rm", stream=lane.handle)
        for i, (tb, _, _) in enumerate(cases):
            n = tb.shape[0]
            dev.trsm(M(lane.live[3 + 2 * i], n), M(lane.live[4 + 2 * i], n), upper=False, right=True, stream=lane.handle)
        return junk_writer(dev, lane, 1 << 20, blocks=2, rounds=150)

    def check(_, outs):
        assert np.array_equal(cut(outs[0][2], first[2]), pk[3])
        for i, (tb, _, x) in enumerate(cases):
            assert np.array_equal(cut(outs[0][4 + 2 * i], tb.shape[0]), x), ("solve", i)

    trim(dev)
    run_pending([[padded(v) for v in pk[:3]] + [padded(v) for tb, b0, _ in cases for v in (g.bits_to_words(tb), b0)]], issue, check)


# ---- 3. two caller streams interleaved from one host thread; 4. gf2_trim ---------------------------------------------------------

STRASSEN, STREAMK = (1280, 2048, 1024), (1000, 1025, 4097)


def lane_operands(seed):
    """operands of one stream: a Strassen product, a stream-K plain product, a triangular solve"""
    ps, pk = product(*STRASSEN, seed), product(*STREAMK, seed + 3)
    tb, b0, x = trsm_case(N_TRSM, 65, True, False, seed + 6)
    return [padded(v) for v in (*ps[:3], *pk[:3], g.bits_to_words(tb), b0)], (ps[3], pk[3] ^ pk[2], x)


def issue_interleaved(dev, pair, strassen=True):
    M = dev.DMat.from_torch
    if strassen:
        for ln in pair:
            dev.mul(M(ln.live[0], STRASSEN[1]), M(ln.live[1], STRASSEN[2]), C=M(ln.live[2], STRASSEN[2]), algo="strassen", param=2,
                    stream=ln.handle)
    for ln in pair:
        dev.mul(M(ln.live[3], STREAMK[1]), M(ln.live[4], STREAMK[2]), C=M(ln.live[5], STREAMK[2]), accumulate=True, algo="m4rm",
                stream=ln.handle)
    for ln in pair:
        dev.trsm(M(ln.live[6], N_TRSM), M(ln.live[7], 65), upper=True, stream=ln.handle)


def check_interleaved(outs, wants, strassen=True):
    for i, (got, want) in enumerate(zip(outs, wants)):
        if strassen:
            assert np.array_equal(cut(got[2], STRASSEN[2]), want[0]), ("Strassen product of stream", i)
        assert np.array_equal(cut(got[5], STREAMK[2]), want[1]), ("stream-K product of stream", i)
        assert np.array_equal(cut(got[7], 65), want[2]), ("triangular solve of stream", i)


def test_two_streams_interleaved(dev):
    """the same shapes with different operands, issued alternately on two streams that both still sleep: arenas of equal size are
    in play, and each stream's results must be its own (scratch keyed by anything but device, stream and slot mixes them)"""
    (in1, want1), (in2, want2) = lane_operands(91), lane_operands(191)
    run_pending([in1, in2], lambda pair: issue_interleaved(dev, pair), lambda _, outs: check_interleaved(outs, (want1, want2)))


def test_trim_then_the_streams_rebuild_their_arenas(dev):
    """gf2_trim at a quiet point erases the arenas of the caller streams too; the same calls on the same streams afterwards"""
    import torch
    (in1, want1), (in2, want2) = lane_operands(91), lane_operands(191)
    pair = lanes(in1, in2)
    for rnd in range(2):
        for ln in pair:
            ln.open()
        issue_interleaved(dev, pair, strassen=False)
        check_interleaved([ln.read() for ln in pair], (want1, want2), strassen=False)
        if rnd == 0:
            trim(dev)
            for ln in pair:
                ln.poison()
            torch.cuda.synchronize()


# ---- 4. stream-ordered and synchronous frees ---------------------------------------------------------------------------------

def pending_product(dev, sleep, seed):
    """C = A*B queued behind the sleep, A and B library blocks (from an empty pool) that the stream itself fills"""
    m, l, n = STREAMK
    a, b, c0, ref = product(m, l, n, seed)  # gf2_dmat_fill_random writes random_words(.., seed) and (.., seed + 1)
    trim(dev)
    (lane,) = lanes([padded(c0)], sleep=sleep)
    A, B = dev.DMat(m, l), dev.DMat(l, n)
    lane.open()
    A.fill_random(seed, lane.handle)
    B.fill_random(seed + 1, lane.handle)
    dev.mul(A, B, C=dev.DMat.from_torch(lane.live[0], n), algo="m4rm", stream=lane.handle)
    return lane, A, B, ref


def junk_blocks(dev, shapes, count=4):
    """fresh library matrices of the given shapes, filled with other bits on a stream of their own that does not sleep"""
    import torch
    s2 = torch.cuda.Stream()
    give_the_pool_a_chance(dev, s2.cuda_stream)
    mats = [dev.DMat(r, c) for _ in range(count) for r, c in shapes]
    for i, X in enumerate(mats):
        X.fill_random(5000 + i, s2.cuda_stream)
    return s2, mats


def test_free_async_keeps_the_block_until_the_stream_has_passed(dev):
    """While the stream has not finished, no new allocation of the same size may get A's or B's block.  (The address check needs the
    stream to be still busy when the allocations are done; on a host too slow for 0.1 s the set-up is repeated with a longer sleep.)"""
    m, l, n = STREAMK
    for sleep in (1, 4, 16):
        lane, A, B, ref = pending_product(dev, sleep, 301)
        old = {A.s.data, B.s.data}
        for X in (A, B):
            free_async(dev, X, lane.handle)
        s2, fresh = junk_blocks(dev, [(m, l), (l, n)])
        new = {X.s.data for X in fresh}
        busy = lane.pending()
        (got,) = lane.read()
        assert np.array_equal(cut(got, n), ref), "the product read a recycled operand"
        if busy:
            assert not (old & new), "a block freed with gf2_dmat_free_async was handed out before its stream had passed the free"
            return
    raise AssertionError("the stream never outlasted the allocations: nothing was checked")


def test_free_waits_for_pending_work(dev):
    """gf2_dmat_free has hipFree's semantics: it returns when the pending product has run, so the block may be reused at once"""
    m, l, n = STREAMK
    for sleep in (1, 4, 16):
        lane, A, B, ref = pending_product(dev, sleep, 311)
        busy = lane.pending()
        dev._lib.lib().gf2_dmat_free(ctypes.byref(A.s))
        assert lane.stream.query(), "gf2_dmat_free returned while work queued on a stream was still pending"
        s2, fresh = junk_blocks(dev, [(m, l)])
        (got,) = lane.read()
        assert np.array_equal(cut(got, n), ref)
        if busy:
            return
    raise AssertionError("the stream never outlasted the host: gf2_dmat_free had nothing to wait for")


def test_python_temporaries_in_a_chain(dev):
    """DMat.__del__: a temporary used on one stream goes through gf2_dmat_free_async (so does the zero matrix inside DMat.clone), a
    matrix used on two streams through gf2_dmat_free"""
    import torch
    m, l, n, q = 1000, 1025, 4097, 300
    a, b, _, ab = product(m, l, n, 11)
    z, w = g.random_words(n, q, 321), g.random_words(m, q, 322)
    y = g.random_words(l, q, 323)
    want = g.o_mul_fast(ab, z, m, n, q) ^ w
    want2 = g.o_mul_fast(g.random_words(m, l, 324), y, m, l, q)
    for sleep in (1, 4, 16):
        trim(dev)
        (lane,) = lanes([padded(x) for x in (a, b, z, w, y, g.random_words(m, q, 325), g.random_words(m, q, 326))], sleep=sleep)
        lane.open()
        t, s = lane.live, lane.handle
        M = dev.DMat.from_torch
        T = dev.mul(M(t[0], l), M(t[1], n), algo="m4rm", stream=s)
        Tc = T.clone(stream=s)
        old = {T.s.data, Tc.s.data}
        del T  # behind the clone that reads it
        U = dev.mul(Tc, M(t[2], q), stream=s)
        old.add(U.s.data)
        del Tc
        dev.add(U, M(t[3], q), C=M(t[5], q), stream=s)
        del U
        s2, fresh = junk_blocks(dev, [(m, n), (m, q)])
        new = {X.s.data for X in fresh}
        busy = lane.pending()
        # a matrix used on two streams: its __del__ must wait for the device
        Mx, side = dev.DMat(m, l), torch.cuda.Stream()
        Mx.fill_random(324, s)
        dev.mul(Mx, M(t[4], q), C=M(t[6], q), stream=s)
        Dj = dev.transpose(Mx, stream=side.cuda_stream)  # (reads whatever Mx holds by then: the result is not looked at)
        assert len(Mx._streams) == 2
        del Mx
        assert lane.stream.query(), "a DMat used on two streams was freed without waiting for them"
        got = lane.read()
        assert np.array_equal(cut(got[5], q), want), "a temporary of the chain was recycled under queued work"
        assert np.array_equal(cut(got[6], q), want2)
        del Dj
        if busy:
            assert not (old & new), "a temporary freed by DMat.__del__ was handed out before its stream had passed the free"
            return
    raise AssertionError("the stream never outlasted the allocations: nothing was checked")


# ---- 5. several host threads on one caller stream ------------------------------------------------------------------------------

def test_three_threads_share_one_stream(dev):
    """multi-launch calls from several host threads on the SAME stream must not interleave (g_enqueue_mu, g_trsm_mu): each thread
    loops over a Strassen product, a stream-K product and a triangular solve with its own operands"""
    import torch
    rounds = 3
    s = torch.cuda.Stream()
    M = dev.DMat.from_torch
    work = []
    for i in range(3):
        ins, want = lane_operands(401 + 20 * i)
        t = [torch.from_numpy(np.array(x).view(np.int64)).cuda() for x in ins]
        outs = [(torch.full_like(t[2], 1), torch.full_like(t[5], 2), t[7].clone()) for _ in range(rounds)]
        work.append((t, outs, (want[0], product(*STREAMK, 401 + 20 * i + 3)[3], want[2])))
    torch.cuda.synchronize()
    errors = []

    def run(t, outs):
        try:
            for c_s, c_k, x in outs:
                dev.mul(M(t[0], STRASSEN[1]), M(t[1], STRASSEN[2]), C=M(c_s, STRASSEN[2]), algo="strassen", param=2, stream=s.cuda_stream)
                dev.mul(M(t[3], STREAMK[1]), M(t[4], STREAMK[2]), C=M(c_k, STREAMK[2]), algo="m4rm", stream=s.cuda_stream)
                dev.trsm(M(t[6], N_TRSM), M(x, 65), upper=True, stream=s.cuda_stream)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t, outs)) for t, outs, _ in work]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    with torch.cuda.stream(s):
        host = [[tuple(o.cpu() for o in trio) for trio in outs] for _, outs, _ in work]
    for i, (rows, (_, _, want)) in enumerate(zip(host, work)):
        for r, trio in enumerate(rows):
            c_s, c_k, x = (h.numpy().view(np.uint64) for h in trio)
            assert np.array_equal(cut(c_s, STRASSEN[2]), want[0]), ("Strassen product", "thread", i, "round", r)
            assert np.array_equal(cut(c_k, STREAMK[2]), want[1]), ("stream-K product", "thread", i, "round", r)
            assert np.array_equal(cut(x, 65), want[2]), ("triangular solve", "thread", i, "round", r)
