"""Every device path on DIRTY INTERNAL SCRATCH, against the oracle.

tests/test_gpu_views.py covers dirty memory the caller owns.  Here the memory is the library's own: the block cache behind DevBuf, the
per-stream arenas of gf2_stream_scratch and gf2_dmat_alloc.  None of it is ever cleared, so every kernel has to write each word it later
reads: the pad word of an even row stride, the rows of a padded or packed operand beyond m, partial-tile slots, index arrays.  A
fresh block from the driver is very probably zero, and that is what a test run mostly sees.

Each case (tests/dirty_pool.py) empties the cache, refills it with blocks that hold a pattern in every word, creates its operands --
their pad words hold the pattern too -- and makes its call on a caller stream.  It asserts, in this order,
  1. the result, bit for bit, against what the suite already trusts (gf2util.o_*, trsm_ref, nullspace_ref, blocks_ref, the fixtures of
     tests/golden): no tolerances; a result the library allocated has zero excess bits; a preallocated result lives in a poisoned
     parent that must come back intact; source operands keep every word, the pad word included;
  2. the kernel family the case is meant for launched (launch census);
  3. no block came fresh from the driver between the seeding and the last check (gf2_dev_alloc_counts), operands and results included;
  4. where the path uses scratch, the cache served at least one request during the call itself.
The index pattern runs first and the random one only after its assertions have passed (see dirty_pool).  Shapes: the smallest the
planner sends down each path.  Five shapes one would expect run elsewhere under the shipped thresholds and were replaced:
  * 100 x 40065 x 2050 (n >= 1024 needs m <= 64 for the transposed few-rows path) -> 100 x 40065 x 1001, still two passes, l odd in words;
  * 2500 x 3000 x 33 takes the slab tables (kept as such); 33-64 vectors reach the wave-per-row kernel's second pass only through
    gf2_mul_nt_dev from 8192 rows of 16384 bits on -> mul_nt 8200 x 16447 x 33 (257 words: Bt has a pad word);
  * 300 x 40000 x 200 takes the tile kernel; two slab passes need 4096 rows of 32768 bits -> 4100 x 33000 x 200;
  * 1030 x 2049 x 2050 with one level is padded, not peeled -> 1024 x 1054 x 8192 (a 30-bit tail of the inner dimension);
  * no fixed shape of test_packed_tile_paths_ragged packs A under the shipped model -> 8200 x 1025 x 4097 (m % 64 = 8).
The module's name sorts before tests/test_zz_kernel_census.py."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import blocks_ref
import dirty_pool as dp
import gf2util as g
import nullspace_ref
import ple_cases
import trsm_ref
from census_util import assert_route, census

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# any request from 9 to 63 MiB finds a block of 1 to 1.25 times its size, twice (an operand and an arena of one size)
LADDER = (10, 12, 15, 18, 22, 27, 33, 41, 51, 63) * 2


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


def golden(*parts):
    return np.load(os.path.join(HERE, "golden", *parts))


# ---- the harness ------------------------------------------------------------------------------------------------------------------------

def counted(pool, fn):
    """-> (fn(), cache hits during the call, census before, census after)"""
    k0, h0 = census(pool.L), pool.hits()
    out = fn()
    h1, k1 = pool.hits(), census(pool.L)
    return out, h1 - h0, k0, k1


def seeded(L, pattern, big):
    """seed() starts with gf2_trim, which waits for the device: an error a kernel of an earlier case left behind surfaces here, and
    nothing more is started on a device in that state"""
    from m4ri_rust_amd._lib import HipError
    try:
        return dp.Pool(L, pattern, LADDER if big else ())
    except HipError as e:
        pytest.exit("the device reports an error left by an earlier case; no further case is started: %s" % e, returncode=3)


def run_case(L, name, body, scratch=True, big=False):
    """body(pool, stream, pad) makes the operands, the call and checks 1 and 2; -> the cache hits counted during the call"""
    import torch
    for pattern in dp.PATTERNS:
        pool = seeded(L, pattern, big)
        stream = torch.cuda.Stream()  # a caller stream; its arenas are new (seed() released every arena)
        hits = body(pool, stream.cuda_stream, dp.pad_word(pattern))
        pool.no_fresh(name)
        print("dirty-workspace %s pattern=%s hits-in-call=%d hits-in-case=%d seed=%.0fms" % (
            name, "index" if pattern == dp.INDEX else "random", hits, pool.hits() - pool.hits0, pool.seed_seconds * 1e3))
        if scratch:
            assert hits >= 1, "%s: the call drew nothing from the cache: it is listed as using scratch" % name


def test_the_seeded_cache_serves_the_pattern_and_the_counters_count(L, dev):
    """the premise of every case below: a block from the seeded cache holds the pattern, a hit counts as a hit, and a request no
    seeded block can serve counts as fresh"""
    for pattern in dp.PATTERNS:
        pool = seeded(L, pattern, False)
        h0 = pool.hits()
        M = dev.DMat(1000, 129)  # 1000 rows of 4 words: a 1 MiB request
        assert pool.hits() == h0 + 1
        got = dp.raw(M)
        if pattern == dp.INDEX:
            assert (got == np.uint64(dp.INDEX)).all()
        else:
            assert len(np.unique(got)) > 0.99 * got.size
        pool.no_fresh("a 1 MiB block")
        nine = dev.DMat(9 * 1024, dp.COLS)  # 9 MiB: the plain seed list ends at 8
        assert dp.counts(L) == (h0 + 1, pool.fresh0 + 1)
        with pytest.raises(AssertionError):
            pool.no_fresh("a 9 MiB block")
        del nine


def result_in_parent(dev, m, n, c0, seed):
    """C as an m x n view at row 1, word 2 of a parent full of random bits (its own region too, unless c0 gives C's words)"""
    w = g.width(n)
    pw = (w + 5) & ~1
    host = g.splitmix64(seed ^ 0xC0FFEE, np.arange((m + 2) * pw, dtype=np.uint64)).reshape(m + 2, pw).copy()
    if c0 is not None:
        host[1:1 + m, 2:2 + w] = c0
    P = dp.dmat(host, pw * 64, 0)
    return P, dev.DMat.wrap(P.s.data + 8 * (pw + 2), m, n, pw, keep=P), host


def check_parent(P, host, want, m, n, stream):
    """the result's words (zero excess bits included) inside, every word of the parent outside as it was"""
    expect = host.copy()
    expect[1:1 + m, 2:2 + g.width(n)] = want
    got = dp.raw(P, stream)
    bad = np.argwhere(got != expect)
    assert not len(bad), "%d wrong words, first at parent (row, word) %s (the result is at row 1, word 2)" % (len(bad), tuple(bad[0]))


def pad_intact(M, pad, ncols, stream):
    """an in-place call leaves the pad word of the matrix's row stride alone"""
    if M.ld > g.width(ncols):
        assert (dp.raw(M, stream)[:, g.width(ncols):] == np.uint64(pad)).all(), "the pad word of the row stride was written"


# ---- products -------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def product_ref(m, l, n, seed):
    a, b, c0 = g.random_words(m, l, seed), g.random_words(l, n, seed + 1), g.random_words(m, n, seed + 2)
    prod = (g.o_mul_fast if max(m, l, n) >= 4096 else g.o_mul_m4rm)(a, b, m, l, n)
    for x in (a, b, c0, prod):
        x.setflags(write=False)
    return a, b, c0, prod


def mul_step(dev, pool, s, pad, m, l, n, algo, param, families, acc, seed):
    a, b, c0, prod = product_ref(m, l, n, seed)
    A, B = dp.dmat(a, l, pad), dp.dmat(b, n, pad)
    P, C, host = result_in_parent(dev, m, n, c0 if acc else None, seed)
    _, hits, k0, k1 = counted(pool, lambda: dev.mul(A, B, C, accumulate=bool(acc), algo=algo, param=param, stream=s))
    check_parent(P, host, prod ^ c0 if acc else prod, m, n, s)
    dp.unchanged(A, s)
    dp.unchanged(B, s)
    assert_route(k0, k1, families)
    return hits


def ws_bytes(L, dev, m, l, n, algo, param=0):
    return L.gf2_mul_workspace_bytes(m, l, n, dev.ALGOS[algo], param)


def even(w):
    return (w + 1) & ~1


# (name, algo, param, m, l, n, kernel families, uses scratch, needs blocks above 8 MiB)
PRODUCTS = [
    ("tile-streamk", "m4rm", 0, 1000, 1025, 4097, ["gf2_m4rm_kernel_v8", "gf2_streamk_reduce_kernel"], True, True),       # slot 1: 20 MiB
    ("splitk-v3", "m4rm", 0, 100, 5001, 97, ["gf2_m4rm_kernel_v3"], True, False),                                         # slot 1
    ("splitk-v6", "m4rm", 0, 6001, 4097, 4097, ["gf2_m4rm_kernel_v6"], True, True),                                       # slot 1: 52 MiB
    ("packed-a", "m4rm", 0, 8200, 1025, 4097, ["gf2_packA_kernel", "gf2_m4rm_kernel_v8"], True, False),                   # slot 2
    ("strassen-aligned", "strassen", 2, 4096, 4096, 4096, ["gf2_strassen_split", "gf2_strassen_merge"], True, True),      # slot 0: 19 MiB
    ("strassen-padded", "strassen", 2, 2113, 2144, 2175, ["gf2_padcopy_kernel", "gf2_strassen_"], True, False),           # slots 0 and 3
    ("strassen-peeled", "strassen", 1, 1024, 1054, 8192, ["gf2_strassen_", "gf2_m4rm_kernel"], True, True),               # slot 0, strip plain
    ("widevec-1", "naive", 0, 3001, 1025, 1, ["gf2_widevec_kernel", "gf2_transpose"], True, False),                       # slot 0: Bt, 17 words
    ("slab-tables-33", "m4rm", 0, 2500, 3000, 33, ["gf2_tallskinny7_kernel"], False, False),
    ("few-rows-t-33", "m4rm", 0, 33, 40065, 2050, ["gf2_tallskinny7_kernel", "gf2_transpose"], True, True),               # slot 0: Bt 627 words
    ("few-rows-t-100", "m4rm", 0, 100, 40065, 1001, ["gf2_tallskinny7_kernel", "gf2_transpose"], True, False),            # two passes: Ct 2 words
    ("few-rows-va", "m4rm", 0, 3, 5000, 300, ["gf2_va_kernel"], False, False),
    ("slab-tables", "naive", 0, 65601, 705, 1, ["gf2_tallskinny7_kernel"], False, False),
    ("slab-passes-1", "m4rm", 0, 3000, 9000, 100, ["gf2_tallskinny7_kernel"], False, False),
    ("slab-passes-2", "m4rm", 0, 4100, 33000, 200, ["gf2_tallskinny7_kernel"], False, True),
    ("lpn8", "m4rm", 0, 20001, 255, 32, ["gf2_lpn8_kernel"], False, False),
    ("lpn256", "m4rm", 0, 20001, 193, 160, ["gf2_lpn256_kernel"], False, False),
    ("lpnvec", "naive", 0, 262401, 255, 1, ["gf2_lpnvec_kernel"], False, True),
    ("narrow", "naive", 0, 5001, 321, 1, ["gf2_narrow_kernel"], False, False),
    ("naive-1000", "naive", 0, 1000, 1000, 1000, ["gf2_m4rm_kernel_v8"], True, False),                                    # slot 1
]


def test_the_planner_still_sends_the_shapes_where_the_cases_say(L, dev):
    """the pad-word geometry and the planner's side of the routes (the census asserts the kernels' side in every case)"""
    assert g.width(1025) % 2 == 1 and g.width(40065) == 627 and g.width(16447) == 257 and g.width(513) % 2 == 1  # Bt has a pad word
    assert ws_bytes(L, dev, 3001, 1025, 1, "naive") == 1 * even(g.width(1025)) * 8                               # wave per row: Bt in slot 0
    for m, l, n in ((33, 40065, 2050), (100, 40065, 1001)):                                                     # computed transposed
        assert ws_bytes(L, dev, m, l, n, "m4rm") == (n * even(g.width(l)) + 2 * l + n * even(g.width(m)) + m * even(g.width(n))) * 8
    out = (ctypes.c_longlong * 9)()
    L.gf2_tile_plan(8200, 1025, 4097, 1, 1, out)
    assert ws_bytes(L, dev, 8200, 1025, 4097, "m4rm") == out[4] + ((8200 + 63) & ~63) * even(g.width(1025)) * 8 and 8200 % 64  # A is packed
    kind, dims = ctypes.c_int(), (ctypes.c_int * 3)()
    for (m, l, n, param), want in (((4096, 4096, 4096, 2), (2, 0)), ((2113, 2144, 2175, 2), (2, 1)), ((1024, 1054, 8192, 1), (1, 2))):
        assert (L.gf2_mul_plan(m, l, n, dev.ALGOS["strassen"], param, ctypes.byref(kind), dims), kind.value) == want, (m, l, n)


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("case", PRODUCTS, ids=[c[0] for c in PRODUCTS])
def test_mul_dev(L, dev, case, acc):
    name, algo, param, m, l, n, families, scratch, big = case
    seed = 100 + PRODUCTS.index(case) * 10
    run_case(L, "%s-%s" % (name, "acc" if acc else "plain"),
             lambda pool, s, pad: mul_step(dev, pool, s, pad, m, l, n, algo, param, families, acc, seed), scratch, big)


def mul_nt_step(dev, pool, s, pad, m, l, n, families, acc, seed):
    a, b, c0, prod = product_ref(m, l, n, seed)
    A, Bt = dp.dmat(a, l, pad), dp.dmat(g.o_transpose(b, l, n), l, pad)
    P, C, host = result_in_parent(dev, m, n, c0 if acc else None, seed)
    _, hits, k0, k1 = counted(pool, lambda: dev.mul_nt(A, Bt, C, accumulate=bool(acc), stream=s))
    check_parent(P, host, prod ^ c0 if acc else prod, m, n, s)
    dp.unchanged(A, s)
    dp.unchanged(Bt, s)
    assert_route(k0, k1, families)
    return hits


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
@pytest.mark.parametrize("l,n", [(65, 1), (65, 65), (513, 1), (513, 65)])
def test_mul_nt_dev(L, dev, l, n, acc):
    run_case(L, "mul-nt-%dx%d-%d" % (l, n, acc),
             lambda pool, s, pad: mul_nt_step(dev, pool, s, pad, 1000, l, n, ["gf2_rowparity_kernel"], acc, 400 + l + n), scratch=False)


@pytest.mark.parametrize("acc", [0, 1], ids=["plain", "accumulate"])
def test_mul_nt_dev_wave_per_row_in_two_passes(L, dev, acc):
    """33 vectors of 257 words: the second pass of the wave-per-row kernel reads Bt from row 32 on, pad words in between"""
    run_case(L, "mul-nt-two-passes-%d" % acc,
             lambda pool, s, pad: mul_nt_step(dev, pool, s, pad, 8200, 16447, 33, ["gf2_widevec_kernel"], acc, 470), scratch=False, big=True)


@pytest.mark.parametrize("m,n", [(63, 65), (1000, 129)])
def test_transpose_into_a_result_of_the_library(L, dev, m, n):
    a = g.random_words(m, n, 480 + m)
    want = g.o_transpose(a, m, n)

    def body(pool, s, pad):
        S = dp.dmat(a, n, pad)
        D, hits, k0, k1 = counted(pool, lambda: dev.transpose(S, stream=s))
        assert np.array_equal(D.to_words(s), want), "the transpose, or excess bits in its last word"
        dp.unchanged(S, s)
        assert_route(k0, k1, ["gf2_transpose"])
        return hits
    run_case(L, "transpose-%dx%d" % (m, n), body)  # (the hit is D itself)


def test_one_chain_on_one_stream(L, dev):
    """Slot 0 is shared by Strassen, the wave-per-row path and the transposed few-rows path: each step finds what the one before left
    in the arena (and mul_nt reads operands created behind them); no re-seeding in between."""
    steps = [(4096, 4096, 4096, "strassen", 2, ["gf2_strassen_"]), (3001, 1025, 1, "naive", 0, ["gf2_widevec_kernel"]),
             (33, 40065, 2050, "m4rm", 0, ["gf2_tallskinny7_kernel", "gf2_transpose"])]

    def body(pool, s, pad):
        hits = 0
        for i, (m, l, n, algo, param, families) in enumerate(steps):
            hits += mul_step(dev, pool, s, pad, m, l, n, algo, param, families, i & 1, 500 + 10 * i)
            pool.no_fresh("chain step %d" % i)
        mul_nt_step(dev, pool, s, pad, 1000, 513, 65, ["gf2_rowparity_kernel"], 0, 540)
        return hits
    run_case(L, "chain", body, big=True)


# ---- elimination family ---------------------------------------------------------------------------------------------------------------

def low_rank(m, n, r, seed):
    return ple_cases.low_rank(m, n, r, seed)


ECHELON = [  # (name, m, n, ncols_limit, input, kernel family, needs blocks above 8 MiB, M4RI_HIP_ELIM_BLOCK_WORDS or None)
    ("single-launch-192x256", 192, 256, 0, lambda: g.random_words(192, 256, 601), "gf2_elim_small_kernel", False, None),
    ("blocked-193x257", 193, 257, 0, lambda: g.random_words(193, 257, 602), "gf2_elim_pivot_kernel", False, None),
    ("blocked-600x520", 600, 520, 0, lambda: g.random_words(600, 520, 603), "gf2_elim_pivot_kernel", False, None),
    ("rank37-300x400", 300, 400, 0, lambda: golden("elim", "rref_lowrank_300x400_r37.npz")["a"], "gf2_elim_pivot_kernel", False, None),
    ("tall-33000x193", 33000, 193, 0, lambda: g.random_words(33000, 193, 605), "gf2_elim_pivot_kernel", True, None),  # U: 33000 x 32 words
    ("augmented-120x113-limit80", 120, 113, 80, lambda: g.random_words(120, 113, 606), "gf2_elim_small_kernel", False, None),
    # the shapes above fit one block of 2048 columns; with blocks of 128 columns the same shapes also run the part between two
    # blocks: the row moves through `tmp`, the copy of the pivot rows into `P` (520 columns: 9 words, `pld` = 10, a pad word) and the
    # trailing product U * P
    ("blocked-600x520-blocks-of-128", 600, 520, 0, lambda: g.random_words(600, 520, 603), "gf2_m4rm_kernel", False, 2),
    ("rank37-300x400-blocks-of-128", 300, 400, 0, lambda: golden("elim", "rref_lowrank_300x400_r37.npz")["a"], "gf2_elim_gather_kernel", False, 2),
]


@pytest.mark.parametrize("full", [1, 0])
@pytest.mark.parametrize("case", ECHELON, ids=[c[0] for c in ECHELON])
def test_echelonize_dev(L, dev, case, full, monkeypatch):
    """full = 0: the upper echelon form is not unique; it must have the oracle's rank and pivots, zero rows below the rank and, reduced
    fully by the oracle, give the oracle's reduced form"""
    name, m, n, limit, make, family, big, block_words = case
    if block_words:
        monkeypatch.setenv("M4RI_HIP_ELIM_BLOCK_WORDS", str(block_words))  # (read per call)
    a = np.ascontiguousarray(make())
    red, orank, opiv = g.o_echelonize(a, m, n, full=True, limit=limit)

    def body(pool, s, pad):
        A = dp.dmat(a, n, pad)
        (rank, piv), hits, k0, k1 = counted(pool, lambda: dev.echelonize(A, full=bool(full), ncols_limit=limit, stream=s))
        got = A.to_words(s)
        assert rank == orank and piv == opiv
        if full:
            assert np.array_equal(got, red), "not the oracle's reduced echelon form"
        else:
            lim = limit if limit else n
            assert not g.words_to_bits(got, n)[rank:, :lim].any()
            again, rank2, _ = g.o_echelonize(got, m, n, full=True, limit=limit)
            assert rank2 == rank and np.array_equal(again[:rank], red[:rank])
            # below the rank only augmented columns are left: each row is its input row reduced by the pivot rows, in some order
            assert sorted(map(bytes, again[rank:])) == sorted(map(bytes, red[rank:]))
        pad_intact(A, pad, n, s)
        assert_route(k0, k1, [family, "gf2_elim_pivot_kernel" if block_words else family])
        return hits
    run_case(L, "echelonize-%s-full%d" % (name, full), body, big=big)


@pytest.mark.parametrize("n,block_words", [(1, None), (65, None), (200, None), (300, 2)])
def test_inverse_dev(L, dev, n, block_words, monkeypatch):
    """up to n = 200 (the fixtures) [A | pad | I] takes the single launch; (300, 2): the blocked elimination in blocks of 128 columns,
    with trailing products over augmented columns that are cut at the last non-zero word"""
    if block_words:
        monkeypatch.setenv("M4RI_HIP_ELIM_BLOCK_WORDS", str(block_words))  # (read per call)
        seed = 611
        while g.o_inverse(g.random_words(n, n, seed), n) is None:
            seed += 1
        a = g.random_words(n, n, seed)
        inv = g.o_inverse(a, n)
    else:
        d = golden("elim", "inverse_%d.npz" % n)
        a, inv = np.ascontiguousarray(d["a"]), d["inv"]
        assert np.array_equal(g.o_inverse(a, n), inv)

    def body(pool, s, pad):
        A = dp.dmat(a, n, pad)
        out, hits, k0, k1 = counted(pool, lambda: dev.inverse(A, stream=s))
        assert out is not None and np.array_equal(out.to_words(s), inv), "the inverse, or excess bits in its last word"
        dp.unchanged(A, s)
        assert_route(k0, k1, ["gf2_set_diag_kernel"] + (["gf2_elim_pivot_kernel", "gf2_m4rm_kernel", "gf2_elim_lastword_kernel"] if block_words
                                                        else ["gf2_elim_small_kernel"]))
        return hits
    run_case(L, "inverse-%d%s" % (n, "-blocks-of-128" if block_words else ""), body)


def test_inverse_dev_singular(L, dev):
    n = 100
    a = low_rank(n, n, 60, 611)
    assert g.o_inverse(a, n) is None

    def body(pool, s, pad):
        A = dp.dmat(a, n, pad)
        out, hits, k0, k1 = counted(pool, lambda: dev.inverse(A, stream=s))
        assert out is None
        dp.unchanged(A, s)
        assert_route(k0, k1, ["gf2_elim_"])
        return hits
    run_case(L, "inverse-singular-100", body)


@pytest.mark.parametrize("name", ["solve_120x80x33", "solve_lowrank_200x150x70_r40"])
def test_solve_left_dev(L, dev, name):
    d = golden("elim", name + ".npz")
    m, n, k = (int(x) for x in d["shape"])
    a = np.ascontiguousarray(d["a"])
    red = g.o_echelonize(a, m, n, full=True)[0]
    for b, x, consistent in ((d["b"], d["x"], True), (d["b_inconsistent"], None, not bool(d["inconsistent"][0]))):
        def body(pool, s, pad, b=b, x=x, consistent=consistent):
            A, B = dp.dmat(a, n, pad), dp.dmat(b, k, pad)
            ok, hits, k0, k1 = counted(pool, lambda: dev.solve_left(A, B, check=True, stream=s))
            assert ok is consistent
            want = g.o_solve_left(a, m, n, np.ascontiguousarray(b), b.shape[0], k)[0] if x is None else x
            if consistent:
                assert np.array_equal(B.to_words(s), want), "B: the solution rows, then zero rows"
            assert np.array_equal(A.to_words(s), red), "A does not hold its reduced echelon form"
            pad_intact(A, pad, n, s)
            pad_intact(B, pad, k, s)
            assert_route(k0, k1, ["gf2_elim_", "gf2_scatter_rows_kernel"])
            return hits
        run_case(L, "solve-left-%s-%s" % (name, "ok" if x is not None else "bad"), body)


NULLSPACE = [("single_workgroup", 140, 130, range(65)), ("blocked", 320, 300, range(1, 300, 2)), ("rank37", 300, 400, None)]


@pytest.mark.parametrize("name,m,n,S", NULLSPACE, ids=[c[0] for c in NULLSPACE])
def test_nullspace_dev(L, dev, name, m, n, S):
    """rank37: d = 363 columns of K, not a multiple of 64"""
    from test_gpu_nullspace import six_checks
    if S is None:
        a0 = low_rank(m, n, 37, 3 * m + n)
        red, rank, piv = g.o_echelonize(a0, m, n, full=True)
        want = nullspace_ref.from_rref(red, piv, n)
        assert n - rank == 363
    else:
        a0, want = nullspace_ref.with_pivots(m, n, S, seed=m)

    def body(pool, s, pad):
        A = dp.dmat(a0, n, pad)
        (K, rank, piv), hits, k0, k1 = counted(pool, lambda: dev.nullspace(A, stream=s))
        six_checks(a0, m, n, K.to_words(s), rank, piv, A.to_words(s), want)
        pad_intact(A, pad, n, s)
        assert_route(k0, k1, ["nullspace_prepare", "nullspace_assemble", "gf2_elim_"])
        return hits
    run_case(L, "nullspace-" + name, body)


@pytest.mark.parametrize("n,k", [(n, k) for n in (65, 513, 1089) for k in (65, 130)])
def test_trsm_dev(L, dev, n, k):
    """T with random bits in its other triangle and on its diagonal; n = 65, 513, 1089: a ragged last block of the inversion"""
    for upper, right in trsm_ref.VARIANTS:
        rows, cols = trsm_ref.b_shape(n, k, right)
        tb = trsm_ref.random_bits(n, n, 700 + n)
        t = g.bits_to_words(trsm_ref.dirty(tb, upper, 701 + n))
        b0 = g.random_words(rows, cols, 702 + n + k)
        want = trsm_ref.solve(trsm_ref.clean(tb, upper), b0, rows, cols, upper, right)

        def body(pool, s, pad):
            T, B = dp.dmat(t, n, pad), dp.dmat(b0, cols, pad)
            _, hits, k0, k1 = counted(pool, lambda: dev.trsm(T, B, upper=upper, right=right, stream=s))
            assert np.array_equal(B.to_words(s), want), trsm_ref.name(upper, right)
            pad_intact(B, pad, cols, s)
            dp.unchanged(T, s)
            assert_route(k0, k1, ["trsm_invert_blocks", "trsm_copy_back"])
            return hits
        run_case(L, "trsm-%s-n%d-k%d" % (trsm_ref.name(upper, right), n, k), body)


PLE = [("63x65", lambda: golden("ple", "random_63x65.npz")["a"], 63, 65), ("rank40-200x150", lambda: golden("ple", "rank40_200x150.npz")["a"], 200, 150),
       ("130x260", lambda: golden("ple", "rank64_130x260.npz")["a"], 130, 260), ("1025x200", lambda: g.random_words(1025, 200, 711), 1025, 200)]


@pytest.mark.parametrize("pluq", [0, 1])
@pytest.mark.parametrize("name,make,m,n", PLE, ids=[c[0] for c in PLE])
def test_ple_dev(L, dev, name, make, m, n, pluq):
    a = np.ascontiguousarray(make())
    orank, oP, oQ, oout = g.o_ple(a, m, n, pluq=bool(pluq))

    def body(pool, s, pad):
        A = dp.dmat(a, n, pad)
        (rank, P, Q), hits, k0, k1 = counted(pool, lambda: dev.ple(A, pluq=bool(pluq), stream=s))
        assert rank == orank and P == list(oP) and Q == list(oQ)
        assert np.array_equal(A.to_words(s), oout)
        pad_intact(A, pad, n, s)
        assert_route(k0, k1, ["ple_panel_scan", "ple_panel_apply"])
        return hits
    run_case(L, "ple-%s-pluq%d" % (name, pluq), body)


@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
def test_apply_p_dev(L, dev, right):
    m, n = 70, 130
    a = g.random_words(m, n, 721)
    size = n if right else m
    rng = random.Random(722 + right)
    perm = [rng.randrange(i, size) for i in range(size)]
    for trans in (False, True):
        want = g.o_apply_p(a, m, n, perm, right=right, trans=trans)

        def body(pool, s, pad):
            A = dp.dmat(a, n, pad)
            _, hits, k0, k1 = counted(pool, lambda: dev.apply_p(A, perm, right=right, trans=trans, stream=s))
            assert np.array_equal(A.to_words(s), want)
            pad_intact(A, pad, n, s)
            assert_route(k0, k1, ["ple_gather"] + (["gf2_transpose"] if right else []))
            return hits
        run_case(L, "apply-p-%s%s" % ("right" if right else "left", "-trans" if trans else ""), body)


def test_pluq_solve_left_dev(L, dev):
    m, n, k = 300, 700, 64
    a = low_rank(m, n, 263, 731)
    b = g.o_mul_naive(a, g.random_words(n, k, 732), m, n, k)
    bfull = np.ascontiguousarray(np.vstack([b, g.random_words(n - m, k, 733)]))
    want, consistent = g.o_solve_left(a, m, n, bfull, n, k)
    assert consistent
    orank, oP, oQ, oout = g.o_ple(a, m, n, pluq=True)

    def body(pool, s, pad):
        A, B = dp.dmat(a, n, pad), dp.dmat(bfull, k, pad)
        rank, P, Q = dev.ple(A, pluq=True, stream=s)
        assert rank == orank and np.array_equal(A.to_words(s), oout)
        ok, hits, k0, k1 = counted(pool, lambda: dev.pluq_solve_left(A, rank, P, Q, B, check=True, stream=s))
        x = B.to_words(s)
        assert ok and np.array_equal(g.o_mul_naive(a, np.ascontiguousarray(x), m, n, k), b), "A X != B"
        assert np.array_equal(x, want), "not the solution with the free variables zero"
        assert np.array_equal(A.to_words(s), oout), "the factorisation changed"
        assert_route(k0, k1, ["ple_gather", "trsm_invert_blocks"])
        return hits
    run_case(L, "pluq-solve-left-300x700x64", body)


@pytest.mark.parametrize("m,ncols,batch", [(64, 64, 9), (100, 130, 5)])
def test_echelonize_batch_dev(L, dev, m, ncols, batch):
    """ranks and pivot columns come back in scratch of the wrapper's, from the seeded cache too: every entry must have been written"""
    from test_gpu_elim_batch import reference
    words = g.random_words(batch * m, ncols, 741 + m)
    ref, oranks, opiv = reference(words, m, ncols)

    def body(pool, s, pad):
        A = dp.dmat(words, ncols, pad)
        (ranks, piv), hits, k0, k1 = counted(pool, lambda: dev.echelonize_batch(A, m, stream=s))
        assert np.array_equal(ranks, oranks) and np.array_equal(piv, opiv)
        assert np.array_equal(A.to_words(s), ref)
        pad_intact(A, pad, ncols, s)
        assert_route(k0, k1, ["gf2_elim_batch_"])
        return hits
    run_case(L, "echelonize-batch-%dx%dx%d" % (m, ncols, batch), body, scratch=False)


@pytest.mark.parametrize("n,batch", [(64, 9), (100, 5)])
def test_inverse_batch_dev(L, dev, n, batch):
    """only the blocks of non-singular matrices are compared: the contract leaves the others untouched"""
    words = g.random_words(batch * n, n, 751 + n)
    invs = [g.o_inverse(np.ascontiguousarray(words[b * n:(b + 1) * n]), n) for b in range(batch)]
    assert any(i is not None for i in invs)

    def body(pool, s, pad):
        A = dp.dmat(words, n, pad)
        (Ainv, singular), hits, k0, k1 = counted(pool, lambda: dev.inverse_batch(A, n, stream=s))
        got = Ainv.to_words(s)
        assert list(singular) == [int(i is None) for i in invs]
        for b, inv in enumerate(invs):
            if inv is not None:
                assert np.array_equal(got[b * n:(b + 1) * n], inv), "block %d, or excess bits in its last word" % b
        dp.unchanged(A, s)
        assert_route(k0, k1, ["gf2_elim_batch_"])
        return hits
    run_case(L, "inverse-batch-%dx%d" % (n, batch), body, scratch=False)


@pytest.mark.parametrize("r1,r2,c1,c2", [(64, 1, 64, 1), (100, 300, 128, 300)])
def test_concat_stack_submatrix_into_results_of_the_library(L, dev, r1, r2, c1, c2):
    a, b = g.random_words(r1, c1, 761), g.random_words(r1, c2, 762)   # concat: r1 x (c1 | c2)
    u, v = g.random_words(r1, c2, 763), g.random_words(r2, c2, 764)   # stack: (r1 ; r2) x c2
    cat = blocks_ref.concat(a, c1, b, c2)
    box = (1, 1, r1, c1 + c2) if c1 + c2 > 65 else (0, 1, r1, c1 + c2)  # an unaligned rectangle that ends at the last column

    def body(pool, s, pad):
        A, B, U, V = dp.dmat(a, c1, pad), dp.dmat(b, c2, pad), dp.dmat(u, c2, pad), dp.dmat(v, c2, pad)
        (C, S, T), hits, k0, k1 = counted(pool, lambda: (dev.concat(A, B, stream=s), dev.stack(U, V, stream=s), None))
        assert np.array_equal(C.to_words(s), cat), "concat, or excess bits in its last word"
        assert np.array_equal(S.to_words(s), blocks_ref.stack(u, v, c2)), "stack, or excess bits in its last word"
        W = dev.submatrix(C, *box, stream=s)
        assert np.array_equal(W.to_words(s), blocks_ref.submatrix(cat, c1 + c2, *box)), "submatrix, or excess bits in its last word"
        for M in (A, B, U, V):
            dp.unchanged(M, s)
        assert_route(k0, k1, ["gf2_copy_block"])
        return hits
    run_case(L, "blocks-%dx(%d|%d)" % (r1, c1, c2), body, scratch=False)


# ---- host entries: the device copies of the operands and every DevBuf come from the seeded cache ----------------------------------------

def run_host_case(L, name, body, big=False):
    """body() makes the call on host matrices and checks it; -> (census before, census after, families)"""
    for pattern in dp.PATTERNS:
        pool = seeded(L, pattern, big)
        k0, h0 = census(L), pool.hits()
        families = body()
        hits = pool.hits() - h0
        assert_route(k0, census(L), families)
        pool.no_fresh(name)
        print("dirty-workspace %s pattern=%s hits-in-call=%d seed=%.0fms" % (
            name, "index" if pattern == dp.INDEX else "random", hits, pool.seed_seconds * 1e3))
        assert hits >= 1, "%s: nothing came from the cache" % name


@pytest.mark.parametrize("entry", ["mzd_mul", "mzd_mul_m4rm", "mzd_mul_naive"])
def test_host_products(L, pkg, entry):
    n = 1000
    a, b, _, prod = product_ref(n, n, n, 800)

    def body():
        A, B = pkg.BinMatrix.from_words(a, n), pkg.BinMatrix.from_words(b, n)
        out = L.mzd_mul_naive(None, A.mzd, B.mzd) if entry == "mzd_mul_naive" else getattr(L, entry)(None, A.mzd, B.mzd, 0)
        assert out
        assert np.array_equal(pkg.BinMatrix(out).to_words(), prod)
        return ["gf2_m4rm_kernel"]
    run_host_case(L, "host-" + entry, body)


def test_host_echelonize(L, pkg):
    m, n = 700, 900
    low = low_rank(m, n, 300, 811)
    red, orank, _ = g.o_echelonize(low, m, n, full=True)

    def body():
        M = pkg.BinMatrix.from_words(low, n)
        assert L.mzd_echelonize(M.mzd, 1) == orank and np.array_equal(M.to_words(), red)
        return ["gf2_elim_"]
    run_host_case(L, "host-mzd_echelonize", body)


def test_host_pluq(L, pkg, dev):
    d = golden("ple", "rank40_200x150.npz")
    m, n = int(d["m"]), int(d["n"])

    def body():
        M = pkg.BinMatrix.from_words(d["a"], n)
        P, Q = dev.Mzp(m), dev.Mzp(n)
        assert L.mzd_pluq(M.mzd, P.ptr, Q.ptr, 0) == int(d["rank"])
        assert P.to_list() == list(d["P"]) and Q.to_list() == list(d["Q"]) and np.array_equal(M.to_words(), d["pluq"])
        return ["ple_panel_scan"]
    run_host_case(L, "host-mzd_pluq", body)


def test_host_kernel_left_pluq(L, pkg):
    from test_gpu_nullspace import six_checks
    m, n = 320, 300
    a0, want = nullspace_ref.with_pivots(m, n, range(1, 300, 2), seed=m)
    _, rank, piv = g.o_echelonize(a0, m, n)

    def body():
        H = pkg.BinMatrix.from_words(a0, n)
        K = pkg.BinMatrix(L.mzd_kernel_left_pluq(H.mzd, 0))
        six_checks(a0, m, n, K.to_words(), rank, piv, H.to_words(), want)
        return ["nullspace_assemble"]
    run_host_case(L, "host-mzd_kernel_left_pluq", body)


def test_host_trsm_upper_left(L, pkg):
    n, k = 300, 200
    tb = trsm_ref.random_bits(n, n, 821)
    t = g.bits_to_words(trsm_ref.dirty(tb, True, 822))
    b0 = g.random_words(n, k, 823)
    want = trsm_ref.solve(trsm_ref.clean(tb, True), b0, n, k, True, False)

    def body():
        T, B = pkg.BinMatrix.from_words(t, n), pkg.BinMatrix.from_words(b0, k)
        L.mzd_trsm_upper_left(T.mzd, B.mzd, 0)
        assert np.array_equal(B.to_words(), want) and np.array_equal(T.to_words(), t)
        return ["trsm_invert_blocks"]
    run_host_case(L, "host-mzd_trsm_upper_left", body)


def test_host_solve_left(L, pkg):
    d = golden("elim", "solve_120x80x33.npz")
    m, n, k = (int(x) for x in d["shape"])
    red = g.o_echelonize(np.ascontiguousarray(d["a"]), m, n, full=True)[0]

    def body():
        A, B = pkg.BinMatrix.from_words(d["a"], n), pkg.BinMatrix.from_words(d["b"], k)
        assert L.mzd_solve_left(A.mzd, B.mzd, 0, 1) == 0
        assert np.array_equal(B.to_words(), d["x"]) and np.array_equal(A.to_words(), red)
        return ["gf2_elim_", "gf2_scatter_rows_kernel"]
    run_host_case(L, "host-mzd_solve_left", body)
