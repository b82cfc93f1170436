"""GPU tests of PLE / PLUQ (gf2_ple.hip) bit for bit against the C oracle (oracle_ple, oracle_apply_p, oracle_solve_left) at
the shapes where the device code branches: many panel chunks (ple_panel_scan / _pivots / _apply), tall matrices, deep column
recursion with shifted L compression, a prescribed rank r1 of the left half at the top split (trsm and ple_compress_*), mid
squares, padded row strides, the PLUQ solve, gf2_apply_p_dev, and calls on a caller's stream.  Every case compares rank, P, Q
and every in-place word."""
import random

import numpy as np
import pytest

import gf2util as g
from ple_cases import low_rank, structured
from stream_util import on_stream

pytestmark = pytest.mark.gpu

CHUNK = 1024  # PANEL_CHUNK of gf2_ple.hip


@pytest.fixture(scope="module")
def dev(built):
    from m4ri_rust_amd import device
    device.require_gpu()
    return device


@pytest.fixture(scope="module")
def lib(dev):
    import m4ri_rust_amd as p
    return p


def same(got, want, what=""):
    assert got[0] == want[0], (what, "rank", got[0], want[0])
    assert np.array_equal(np.asarray(got[1]), want[1]), (what, "P differs")
    assert np.array_equal(np.asarray(got[2]), want[2]), (what, "Q differs")
    assert np.array_equal(got[3], want[3]), (what, "in-place result differs")


def dev_ple(dev, a, n, pluq):
    A = dev.DMat.from_words(a, n)
    r, P, Q = dev.ple(A, pluq=pluq)
    return r, P, Q, A.to_words()


def host_ple(lib, a, m, n, pluq):
    from m4ri_rust_amd import device
    L = lib._lib.lib()
    M = lib.BinMatrix.from_words(a, n)
    P, Q = device.Mzp(m), device.Mzp(n)
    r = (L.mzd_pluq if pluq else L.mzd_ple)(M.mzd, P.ptr, Q.ptr, 0)
    return r, P.to_list(), Q.to_list(), M.to_words()


def check(dev, a, m, n, modes=(False, True), what=""):
    for pluq in modes:
        same(dev_ple(dev, a, n, pluq), g.o_ple(a, m, n, pluq), (what, m, n, pluq))


def bits_at(m, n, rows, cols):
    """m x n words with bit (rows[t], cols[t]) set"""
    b = np.zeros((m, n), dtype=np.uint8)
    b[rows, cols] = 1
    return g.bits_to_words(b)


# ---- panel merge: one word column over many chunks ---------------------------------------------------------------------

def panel_cases(m, n):
    yield "random", g.random_words(m, n, m + n)
    base = g.random_words(64, n, 7 * n)
    yield "the same 64 rows in every chunk", np.ascontiguousarray(np.tile(base, (m // 64 + 1, 1))[:m])
    tail = np.zeros((m, g.width(n)), dtype=np.uint64)
    tail[m - 70:] = g.random_words(70, n, m)
    yield "only the last 70 rows", tail
    at = [r for r in (CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK) if r < m]
    a = bits_at(m, n, at, [(1, 0, 3, 2)[t] % n for t in range(len(at))])
    yield "independent rows at the chunk edges", a
    full = g.random_words(m, n, 3 * m)
    k = min(m, n)
    full[:k] = bits_at(k, n, np.arange(k)[::-1], np.arange(k))
    yield "full rank inside chunk 0", full


@pytest.mark.parametrize("m", [1024, 1025, 2047, 4097, 65537, 300001])
@pytest.mark.parametrize("n", [1, 63, 64])
def test_panel_merge(dev, m, n):
    for what, a in panel_cases(m, n):
        check(dev, a, m, n, what=what)


def test_panel_merge_host_entry(dev, lib):
    for m, n in ((2047, 63), (4097, 64)):
        for what, a in panel_cases(m, n):
            for pluq in (False, True):
                same(host_ple(lib, a, m, n, pluq), g.o_ple(a, m, n, pluq), (what, m, n, pluq))


# ---- tall: many chunks under every panel of a recursive factorisation ----------------------------------------------------

@pytest.mark.parametrize("m", [65537, 300001])
@pytest.mark.parametrize("n", [65, 129, 200])
def test_tall(dev, m, n):
    check(dev, g.random_words(m, n, m ^ n), m, n, what="full rank")
    check(dev, low_rank(m, n, 70, n), m, n, what="rank 70")


# ---- deep and wide: about 11 levels of column recursion, L compression with a shift ---------------------------------------

def deep_wide(m, n, seed):
    """rows of an echelon matrix whose leading columns are spread at random outside all-zero column blocks, each row mixed with
    random later rows: the left rank at most nodes is not a multiple of 64"""
    rng = np.random.default_rng(seed)
    zero = np.zeros(n, dtype=bool)
    zero[n // 7:n // 7 + 9000] = True  # an all-zero block inside the matrix
    zero[n - 3000:] = True             # and at its right edge
    zero[2 * n // 3:2 * n // 3 + 640] = True  # whole words
    free = np.nonzero(~zero)[0]
    lead = np.sort(rng.choice(free, size=m, replace=False))
    e = g.words_to_bits(g.random_words(m, n, seed), n)
    e[:, zero] = 0
    e[np.arange(n)[None, :] < lead[:, None]] = 0
    e[np.arange(m), lead] = 1
    mix = np.tril(rng.integers(0, 2, size=(m, m), dtype=np.uint8))
    mix[np.arange(m), np.arange(m)] = 1
    a = g.o_mul_fast(g.bits_to_words(mix), g.bits_to_words(e), m, m, n)
    return np.ascontiguousarray(a[rng.permutation(m)])


@pytest.mark.parametrize("m", [10, 64, 130])
@pytest.mark.parametrize("n", [70000, (1 << 17) + 1])
def test_deep_and_wide(dev, lib, m, n):
    a = deep_wide(m, n, m + n)
    check(dev, a, m, n)
    a2 = g.random_words(m, n, m * 3 + n)
    a2[:, 16:1100] = 0  # zero words in the left panels: the first nodes have r1 = 0
    check(dev, a2, m, n, modes=(True,), what="random with zero column block")
    if m == 130:
        for pluq in (False, True):
            same(host_ple(lib, a, m, n, pluq), g.o_ple(a, m, n, pluq), ("host entry", pluq))


# ---- a prescribed rank r1 of the left half at the top split --------------------------------------------------------------

def top_split(n):
    """cmid of ple_rec's top node"""
    return 64 * ((g.width(n) + 1) // 2)


@pytest.mark.parametrize("r1", [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193])
def test_prescribed_left_rank(dev, lib, r1):
    for j, n in enumerate((512, 1000, 4160)):
        m = (1500, 4097)[(j + r1) % 2]
        cmid = top_split(n)
        assert cmid == {512: 256, 1000: 512, 4160: 2112}[n]
        a = np.ascontiguousarray(np.hstack([low_rank(m, cmid, r1, r1 + n), g.random_words(m, n - cmid, r1 * n + 1)]))
        assert g.o_ple(a[:, :cmid // 64].copy(), m, cmid)[0] == r1
        check(dev, a, m, n, what=("r1", r1))
        if j == 0 and r1 in (0, 65, 193):
            same(host_ple(lib, a, m, n, True), g.o_ple(a, m, n, True), ("host entry", r1))


# ---- mid squares -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2048, 4161, 8192])
def test_mid_squares(dev, n):
    check(dev, g.random_words(n, n, n), n, n, what="random")
    for t, r in enumerate((n - 1, n // 2, 64 * (n // 128) + 1)):
        # one mode per rank at 8192 keeps the oracle's time down; both at the smaller sizes
        modes = ((False, True)[t % 2],) if n == 8192 else (False, True)
        check(dev, low_rank(n, n, r, r), n, n, modes=modes, what=("rank", r))


def test_structured_4096(dev, lib):
    n = 4096
    for t, a in enumerate(structured(n, n)):
        check(dev, a, n, n, what=("structured", t))
        if t in (2, 6):
            same(host_ple(lib, a, n, n, False), g.o_ple(a, n, n, False), ("host entry structured", t))


# ---- padded strides ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(3000, 200), (1025, 64), (700, 4160)])
def test_padded_stride(dev, m, n):
    import torch
    w = g.width(n)
    ld = w + (w & 1) + 2
    a = low_rank(m, n, min(m, n) - 5, m)
    pad = g.random_words(m, (ld - w) * 64, 5 + m)
    for pluq in (False, True):
        t = torch.from_numpy(np.hstack([a, pad]).view(np.int64)).cuda()
        A = dev.DMat.from_torch(t, n)
        r, P, Q = dev.ple(A, pluq=pluq)
        torch.cuda.synchronize()
        got = t.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:, w:], pad), "pad words changed"
        same((r, P, Q, np.ascontiguousarray(got[:, :w])), g.o_ple(a, m, n, pluq), ("padded", m, n, pluq))


def test_dirty_window_over_several_chunks(dev, lib):
    L = lib._lib.lib()
    m, n, r0, c0 = 3000, 200, 5, 64
    pc = c0 + n + 70
    w = g.width(pc)
    for pluq in (False, True):
        parent = lib.BinMatrix.from_words(g.random_words(r0 + m + 3, pc, 41), pc)
        parent._words_view()[:, :w] = g.splitmix64(42 + pluq, np.arange((r0 + m + 3) * w, dtype=np.uint64)).reshape(-1, w)
        before = g.words_to_bits(parent.to_words(), w * 64)
        a = g.bits_to_words(before[r0:r0 + m, c0:c0 + n].copy())
        Wn = L.mzd_init_window(parent.mzd, r0, c0, r0 + m, c0 + n)
        from m4ri_rust_amd import device
        P, Q = device.Mzp(m), device.Mzp(n)
        rank = (L.mzd_pluq if pluq else L.mzd_ple)(Wn, P.ptr, Q.ptr, 0)
        L.mzd_free(Wn)
        after = g.words_to_bits(parent.to_words(), w * 64)
        mask = np.ones_like(after, dtype=bool)
        mask[r0:r0 + m, c0:c0 + n] = False
        assert np.array_equal(after[mask], before[mask]), "parent changed outside the window"
        got = (rank, P.to_list(), Q.to_list(), g.bits_to_words(after[r0:r0 + m, c0:c0 + n].copy()))
        same(got, g.o_ple(a, m, n, pluq), ("dirty window", pluq))


# ---- the PLUQ solve against oracle_solve_left ------------------------------------------------------------------------------

SOLVE = [  # m, n, rank, k
    (4097, 4097, 4097, 64), (4097, 4097, 4096, 65), (4097, 4097, 0, 63),
    (3000, 5000, 65, 1000), (3000, 5000, 2999, 1), (3000, 5000, 3000, 64),
    (5000, 3000, 3000, 63), (5000, 3000, 1, 65), (5000, 3000, 2999, 1000),
    (1025, 64, 64, 5000), (1025, 64, 63, 1), (1025, 64, 0, 65),
    (64, 1025, 64, 1000), (64, 1025, 1, 5000), (64, 1025, 63, 63),
]


def solve_inputs(m, n, r, k, consistent, seed):
    a = low_rank(m, n, r, seed)
    b = g.o_mul_fast(a, g.random_words(n, k, seed + 2), m, n, k) if consistent else g.random_words(m, k, seed + 3)
    brows = max(m, n) + 9  # rows beyond max(m, n): dirty on entry, zero on return
    return a, np.vstack([b, g.random_words(brows - m, k, seed + 4)]), brows


def dev_solve(dev, a, m, n, bfull, k, check):
    A = dev.DMat.from_words(a, n)
    rank, P, Q = dev.ple(A, pluq=True)
    B = dev.DMat.from_words(bfull, k)
    ok = dev.pluq_solve_left(A, rank, P, Q, B, check=check)
    return ok, B.to_words()


def host_solve(lib, a, m, n, bfull, k, check):
    from m4ri_rust_amd import device
    L = lib._lib.lib()
    A, B = lib.BinMatrix.from_words(a, n), lib.BinMatrix.from_words(bfull, k)
    P, Q = device.Mzp(m), device.Mzp(n)
    rank = L.mzd_pluq(A.mzd, P.ptr, Q.ptr, 0)
    rc = L.mzd_pluq_solve_left(A.mzd, rank, P.ptr, Q.ptr, B.mzd, 0, check)
    assert rc in (0, -1)
    return rc == 0, B.to_words()


@pytest.mark.parametrize("m,n,r,k", SOLVE)
def test_pluq_solve_against_oracle(dev, lib, m, n, r, k):
    seed = m + 3 * n + 5 * r + 7 * k
    a, bfull, brows = solve_inputs(m, n, r, k, True, seed)
    want, ok = g.o_solve_left(a, m, n, bfull, brows, k)
    assert ok
    entry = (dev_solve, host_solve)[seed % 2]
    for check in (1, 0):
        got_ok, x = entry(dev if entry is dev_solve else lib, a, m, n, bfull, k, check)
        assert got_ok, ("a consistent system reported inconsistent", check)
        assert np.array_equal(x, want), ("X differs from oracle_solve_left", check)
    if r < m:
        a, bbad, brows = solve_inputs(m, n, r, k, False, seed)
        assert not g.o_solve_left(a, m, n, bbad, brows, k)[1]
        for entry, ctx in ((dev_solve, dev), (host_solve, lib)):
            assert not entry(ctx, a, m, n, bbad, k, 1)[0], "an inconsistent system was not reported"


# ---- gf2_apply_p_dev against oracle_apply_p --------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(70001, 130), (1500, 12000)])
def test_apply_p_against_oracle(dev, m, n):
    rng = random.Random(m + n)
    a = g.random_words(m, n, m * 7 + n)
    for right in (False, True):
        size = n if right else m
        for length in (size, size // 3):  # len < rows (columns): the tail stays in place
            perm = [rng.randrange(i, size) for i in range(length)]
            for trans in (False, True):
                D = dev.DMat.from_words(a, n)
                dev.apply_p(D, perm, right=right, trans=trans)
                want = g.o_apply_p(a, m, n, perm, right=right, trans=trans)
                assert np.array_equal(D.to_words(), want), (right, trans, length)


# ---- calls on a caller's stream ------------------------------------------------------------------------------------------

def test_ple_on_caller_stream(dev):
    for m, n in ((65537, 63), (4096, 4096)):
        w = g.width(n)
        ld = w + (w & 1)
        a = low_rank(m, n, min(m, n) - 3, m + 1) if n > 64 else g.random_words(m, n, 9)
        if n <= 64:
            a[:m - 70] = 0  # pivots only in the last chunk
        src = np.hstack([a, np.zeros((m, ld - w), dtype=np.uint64)])
        for pluq in (False, True):
            res, (out,) = on_stream(dev, [src], lambda t, s: dev.ple(dev.DMat.from_torch(t[0], n), pluq=pluq, stream=s))
            same((*res, np.ascontiguousarray(out[:, :w])), g.o_ple(a, m, n, pluq), ("stream", m, n, pluq))


def test_solve_on_caller_stream(dev):
    m, n, k = 3000, 2500, 100
    a, bfull, brows = solve_inputs(m, n, 2400, k, True, 17)
    want, ok = g.o_solve_left(a, m, n, bfull, brows, k)
    assert ok
    w, kw = g.width(n), g.width(k)
    srcs = [np.hstack([a, np.zeros((m, (w & 1)), dtype=np.uint64)]), np.hstack([bfull, np.zeros((brows, kw & 1), dtype=np.uint64)])]

    def call(t, s):
        A, B = dev.DMat.from_torch(t[0], n), dev.DMat.from_torch(t[1], k)
        rank, P, Q = dev.ple(A, pluq=True, stream=s)
        return dev.pluq_solve_left(A, rank, P, Q, B, check=True, stream=s)

    ok, (_, x) = on_stream(dev, srcs, call)
    assert ok
    assert np.array_equal(np.ascontiguousarray(x[:, :kw]), want)
