"""Device paths on windows of DIRTY parents: every word of the parent holds random bits, the excess bits of each row's last word
included, so a window whose column end is not a multiple of 64 shares its last word with bits that are not its own.  The drop-in
entry points copy whole words to the device (to_device_rows / upload_rows_async), and the device layout promises zero excess bits
only by the masks inside each kernel: a kernel that dropped its output mask, or an upload that took the parent's bits for the
window's, passes every test built with from_words / mzd_randomize (both clear those bits) and fails here.

Every case checks, bit for bit, against the oracle applied to a clean copy of each view's bits:
  1. the bits of the result;  2. a result that is not a window has zero excess bits;  3. a destination window leaves every bit of
  its parent outside the window as it was;  4. source windows and their parents are unchanged;  5. the kernel family the case is
  meant for ran (launch census before and after the call), so that a moved threshold fails the case instead of re-routing it.
Shapes were picked with the shipped planner (gf2_tile_plan, gf2_mul_plan; plain_path's thresholds for the thin products)."""
import numpy as np
import pytest

import gf2util as g
from census_util import assert_route, census

pytestmark = pytest.mark.gpu

R0, C0 = 5, 64  # every window starts below the parent's first row and right of its first word


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


# ---- operands ----------------------------------------------------------------------------------------

def dirty_parent(pkg, nrows, ncols, seed):
    """Random bits in every word of every row, the excess bits of the last word included."""
    P = pkg.BinMatrix.from_words(g.random_words(nrows, ncols, seed), ncols)
    w = g.width(ncols)
    P._words_view()[:, :w] = g.splitmix64(seed ^ 0xD1B54A32D192ED03, np.arange(nrows * w, dtype=np.uint64)).reshape(nrows, w)
    return P


class View:
    """rows x cols operand: a window [R0:R0+rows, C0:C0+cols] of a dirty parent, or a plain (clean) matrix."""

    def __init__(self, pkg, rows, cols, seed, window, extra_cols=70):
        self.L = pkg._lib.lib()
        self.rows, self.cols, self.window = rows, cols, window
        if window:
            self.pcols = C0 + cols + extra_cols
            self.parent = dirty_parent(pkg, R0 + rows + 3, self.pcols, seed)
            self.ptr = self.L.mzd_init_window(self.parent.mzd, R0, C0, R0 + rows, C0 + cols)
            self.ptr._owner = self.parent
        else:
            self.parent = pkg.BinMatrix.from_words(g.random_words(rows, cols, seed), cols)
            self.pcols = cols
            self.ptr = self.parent.mzd

    def raw_bits(self):
        """every bit of the parent's row words, excess bits included"""
        return g.words_to_bits(self.parent.to_words(), g.width(self.pcols) * 64)

    def bits(self):
        """clean words of the view"""
        b = self.raw_bits()
        return g.bits_to_words(b[R0:R0 + self.rows, C0:C0 + self.cols]) if self.window else g.bits_to_words(b[:, :self.cols])

    def free(self):
        if self.window:
            self.L.mzd_free(self.ptr)


def check_result(pkg, C, out, want, m, n, before_c):
    """Contract 1-3 for a result `out` (C: the destination View or None)."""
    if C is None or not C.window:
        R = pkg.BinMatrix(out) if C is None else C.parent
        w = R.to_words()
        if n % 64:
            assert not (w[:, -1] >> np.uint64(n % 64)).any(), "excess bits of a result that is not a window are not zero"
            w[:, -1] &= np.uint64((1 << (n % 64)) - 1)
        assert np.array_equal(w, want), "result bits differ from the oracle"
    else:
        expect = before_c.copy()
        expect[R0:R0 + m, C0:C0 + n] = g.words_to_bits(want, n)
        got = C.raw_bits()
        bad = np.argwhere(got != expect)
        assert not len(bad), "destination window: %d wrong bits, first at parent (row, col) %s" % (len(bad), tuple(bad[0]))


def check_product(pkg, call, m, l, n, win, families, acc=False, seed=1, clean_ref=None):
    """call(C, A, B) -> mzd_t*: C (+)= A * B with the operands named in `win` as windows of dirty parents."""
    L = pkg._lib.lib()
    A, B = View(pkg, m, l, seed, "A" in win), View(pkg, l, n, seed + 1, "B" in win)
    C = View(pkg, m, n, seed + 2, "C" in win) if ("C" in win or acc) else None
    a, b = A.bits(), B.bits()
    prod = clean_ref(a, b) if clean_ref else (g.o_mul_fast if max(m, l, n) >= 4096 else g.o_mul_m4rm)(a, b, m, l, n)
    want = prod ^ C.bits() if acc else prod
    ra, rb = A.raw_bits(), B.raw_bits()
    rc = C.raw_bits() if C is not None else None
    c0 = census(L)
    out = call(C.ptr if C is not None else None, A.ptr, B.ptr)
    c1 = census(L)
    assert out, "the entry point failed"
    check_result(pkg, C, out, want, m, n, rc)
    assert np.array_equal(A.raw_bits(), ra) and np.array_equal(B.raw_bits(), rb), "a source or its parent changed"
    assert_route(c0, c1, families)
    for v in (A, B, C):
        if v is not None:
            v.free()


WINDOWS = ["A", "B", "C", "Cacc", "ABC"]


def _mul_entry(L, kind, acc):
    if kind == "m4rm":
        return (lambda C, A, B: L.mzd_addmul_m4rm(C, A, B, 0)) if acc else (lambda C, A, B: L.mzd_mul_m4rm(C, A, B, 0))
    if kind == "naive":
        return (lambda C, A, B: L.mzd_addmul_naive(C, A, B)) if acc else (lambda C, A, B: L.mzd_mul_naive(C, A, B))
    cutoff = int(kind.split(":")[1])  # "strassen:<cutoff>": forced levels (levels_from_cutoff)
    return (lambda C, A, B: L.mzd_addmul(C, A, B, cutoff)) if acc else (lambda C, A, B: L.mzd_mul(C, A, B, cutoff))


# (route, entry, m, l, n, kernel families that must launch).  Column ends of the windows: l % 64 and n % 64 in {1, 32, 63}, or 0
# (a 64-aligned window narrower than its parent's rows: the 2-D copy path)
ROUTES = [
    ("v8-whole-rounds", "m4rm", 257, 65, 65, ["gf2_m4rm_kernel_v8"]),                         # gf2_tile_plan: variant 12, no cut
    ("v8-streamk", "m4rm", 1000, 1025, 4097, ["gf2_m4rm_kernel_v8", "gf2_streamk_reduce_kernel"]),  # variant 11, 9 tiles cut
    ("v3-splitk", "m4rm", 100, 5001, 97, ["gf2_m4rm_kernel_v3"]),                             # variant 20, 39 slices of l
    ("v6-splitk", "m4rm", 6001, 4097, 4097, ["gf2_m4rm_kernel_v6"]),                          # variant 8, 17 slices of l
    ("strassen-padded", "strassen:1024", 2113, 2144, 2175, ["gf2_padcopy_kernel", "gf2_strassen_"]),  # gf2_mul_plan(.., 2, 1): kind 1
    ("strassen-aligned", "strassen:1024", 4096, 4096, 4096, ["gf2_strassen_"]),               # two forced levels, 64-aligned windows
    ("narrow", "naive", 5001, 321, 1, ["gf2_narrow_kernel"]),                                 # n <= 8, < 262144 rows
    ("lpnvec", "naive", 262401, 255, 1, ["gf2_lpnvec_kernel"]),                               # 1-4 vectors, 64 < l <= 256
    ("lpn8", "m4rm", 20001, 255, 32, ["gf2_lpn8_kernel"]),                                    # tallskinny path, l <= 256, n <= 64
    ("lpn256", "m4rm", 20001, 193, 160, ["gf2_lpn256_kernel"]),                               # 128 < n <= 256
    ("tallskinny3", "m4rm", 524289, 321, 96, ["gf2_tallskinny3_kernel"]),                     # 256 < l <= 1024, n > 64, >= 2^19 rows
    ("tallskinny7", "naive", 65601, 705, 1, ["gf2_tallskinny7_kernel"]),                      # slab tables: >= 65536 rows, l <= 2048
    ("tallskinny7-wide", "m4rm", 3001, 2113, 32, ["gf2_tallskinny7_kernel"]),                 # 17-64 vectors, l >= 2048
    ("widevec", "naive", 3001, 1025, 1, ["gf2_widevec_kernel"]),                              # n <= 8, l >= 768, <= 131072 rows
]


@pytest.mark.parametrize("win", WINDOWS)
@pytest.mark.parametrize("route,kind,m,l,n,families", ROUTES, ids=[r[0] for r in ROUTES])
def test_product_on_dirty_windows(pkg, route, kind, m, l, n, families, win):
    L = pkg._lib.lib()
    acc = win == "Cacc"
    wins = "C" if acc else win
    check_product(pkg, _mul_entry(L, kind, acc), m, l, n, wins, families, acc=acc, seed=1 + 10 * [r[0] for r in ROUTES].index(route))


@pytest.mark.parametrize("win", ["A", "B", "C", "ABC"])
@pytest.mark.parametrize("clear", [1, 0])
def test_mul_naive_pretransposed_on_dirty_windows(pkg, win, clear):
    """_mzd_mul_naive: C (+)= A * Bt^T with Bt given transposed (n x l): the row-parity kernel."""
    L = pkg._lib.lib()
    m, l, n = 3001, 1025, 97
    call = lambda C, A, Bt: L._mzd_mul_naive(C, A, Bt, clear)  # noqa: E731
    wins = win if clear else win + "C"  # accumulating: into a window of a dirty parent
    A, Bt = View(pkg, m, l, 31, "A" in wins), View(pkg, n, l, 32, "B" in wins)
    C = View(pkg, m, n, 33, "C" in wins)
    prod = g.o_mul_m4rm(A.bits(), g.o_transpose(Bt.bits(), n, l), m, l, n)
    want = prod if clear else prod ^ C.bits()
    ra, rb, rc = A.raw_bits(), Bt.raw_bits(), C.raw_bits()
    c0 = census(L)
    assert call(C.ptr, A.ptr, Bt.ptr)
    c1 = census(L)
    if C.window:
        check_result(pkg, C, C.ptr, want, m, n, rc)
    else:
        w = C.parent.to_words()
        assert not (w[:, -1] >> np.uint64(n % 64)).any() and np.array_equal(w, want)
    assert np.array_equal(A.raw_bits(), ra) and np.array_equal(Bt.raw_bits(), rb)
    assert_route(c0, c1, ["gf2_rowparity_kernel"])
    for v in (A, Bt, C):
        v.free()


@pytest.mark.parametrize("win", ["v", "A", "C", "Cacc", "vAC"])
def test_mul_va_on_dirty_windows(pkg, win):
    """_mzd_mul_va: C (+)= v * A with v a ONE-ROW window (the v*A kernel, m <= 8)."""
    L = pkg._lib.lib()
    acc = win == "Cacc"
    call = (lambda C, v, A: L._mzd_mul_va(C, v, A, 0)) if acc else (lambda C, v, A: L._mzd_mul_va(C, v, A, 1))
    # v plays the part of A (1 x l), A that of B (l x n); C is preallocated: a clean matrix unless it is a window
    names = ("A" if "v" in win else "") + ("B" if win in ("A", "vAC") else "") + ("C" if "C" in win else "")
    m, l, n = 1, 1025, 2017
    V, A = View(pkg, m, l, 41, "A" in names), View(pkg, l, n, 42, "B" in names)
    C = View(pkg, m, n, 43, "C" in names)
    prod = g.o_mul_m4rm(V.bits(), A.bits(), m, l, n)
    want = prod ^ C.bits() if acc else prod
    rv, ra, rc = V.raw_bits(), A.raw_bits(), C.raw_bits()
    c0 = census(L)
    assert call(C.ptr, V.ptr, A.ptr)
    c1 = census(L)
    if C.window:
        check_result(pkg, C, C.ptr, want, m, n, rc)
    else:
        w = C.parent.to_words()
        assert not (w[:, -1] >> np.uint64(n % 64)).any() and np.array_equal(w, want)
    assert np.array_equal(V.raw_bits(), rv) and np.array_equal(A.raw_bits(), ra)
    assert_route(c0, c1, ["gf2_va_kernel"])
    for x in (V, A, C):
        x.free()


@pytest.mark.parametrize("dst", ["fresh", "prealloc", "window"])
def test_transpose_of_a_dirty_window(pkg, dst):
    """mzd_transpose of a window source of >= 2^24 bits (the device transposition); a window destination takes the host loop."""
    L = pkg._lib.lib()
    m, n = 4097, 4161
    S = View(pkg, m, n, 51, True)
    want = g.o_transpose(S.bits(), m, n)
    rs = S.raw_bits()
    D = View(pkg, n, m, 52, True) if dst == "window" else (View(pkg, n, m, 52, False) if dst == "prealloc" else None)
    rd = D.raw_bits() if D is not None else None
    c0 = census(L)
    out = L.mzd_transpose(D.ptr if D is not None else None, S.ptr)
    c1 = census(L)
    assert out
    check_result(pkg, D, out, want, n, m, rd)
    assert np.array_equal(S.raw_bits(), rs)
    if dst != "window":
        assert_route(c0, c1, ["gf2_transpose"])
    for v in (S, D):
        if v is not None:
            v.free()


def _outside_unchanged(V, before):
    got = V.raw_bits()
    mask = np.ones_like(got, dtype=bool)
    mask[R0:R0 + V.rows, C0:C0 + V.cols] = False
    assert np.array_equal(got[mask], before[mask]), "a bit of the parent outside the window changed"


@pytest.mark.parametrize("m,n", [(300, 257), (2001, 2113), (20000, 1025)])
@pytest.mark.parametrize("full", [0, 1])
def test_echelonize_dirty_window(pkg, m, n, full):
    """mzd_echelonize on a window: the echelon form inside, the parent's bits outside untouched.  Small (one-workgroup kernel),
    blocked, and tall (the early publication of test_gpu_elim.py's tall cases).  full = 0: the upper echelon form is not unique;
    it must have the oracle's rank and, reduced fully, give the oracle's reduced form."""
    L = pkg._lib.lib()
    W = View(pkg, m, n, 61 + m, True)
    a = W.bits()
    red, orank, _ = g.o_echelonize(a, m, n, full=True)
    before = W.raw_bits()
    c0 = census(L)
    rank = L.mzd_echelonize(W.ptr, full)
    c1 = census(L)
    assert rank == orank
    if full:
        check_result(pkg, W, W.ptr, red, m, n, before)
    else:
        _outside_unchanged(W, before)
        got = W.bits()
        assert not g.words_to_bits(got, n)[rank:].any()
        again, rank2, _ = g.o_echelonize(got, m, n, full=True)
        assert rank2 == rank and np.array_equal(again, red)
    assert_route(c0, c1, ["gf2_elim_"])
    W.free()


def test_inverse_window_into_window(pkg):
    L = pkg._lib.lib()
    n = 1000
    while True:
        S = View(pkg, n, n, 71, True)
        inv = g.o_inverse(S.bits(), n)
        if inv is not None:
            break
        n += 1
    D = View(pkg, n, n, 72, True)
    rs, rd = S.raw_bits(), D.raw_bits()
    c0 = census(L)
    assert L.mzd_inv_m4ri(D.ptr, S.ptr, 0)
    c1 = census(L)
    check_result(pkg, D, D.ptr, inv, n, n, rd)
    assert np.array_equal(S.raw_bits(), rs)
    assert_route(c0, c1, ["gf2_elim_"])
    S.free()
    D.free()


@pytest.mark.parametrize("check", [0, 1])
@pytest.mark.parametrize("consistent", [True, False])
def test_solve_left_on_dirty_windows(pkg, check, consistent):
    """mzd_solve_left(A, B): A and B windows of dirty parents; A X = B with X into B's window (A is left holding an echelon form,
    inside its window only).  A square and singular (rank 600): a consistent B = A X0, an inconsistent random B."""
    L = pkg._lib.lib()
    m, n, k = 700, 700, 97
    A = View(pkg, m, n, 81, True)
    B = View(pkg, m, k, 82, True)
    a = g.o_mul_m4rm(g.random_words(m, 600, 83), g.random_words(600, n, 84), m, 600, n)
    b = g.o_mul_m4rm(a, g.random_words(n, k, 85), m, n, k) if consistent else B.bits()
    for V, w, cols in ((A, a, n), (B, b, k)):  # write the operands into the windows, the parents' other bits as they were
        full = V.raw_bits()
        full[R0:R0 + V.rows, C0:C0 + cols] = g.words_to_bits(w, cols)
        V.parent._words_view()[:, :g.width(V.pcols)] = g.bits_to_words(full)[:, :g.width(V.pcols)]
    assert np.array_equal(A.bits(), a) and np.array_equal(B.bits(), b)
    _, ok = g.o_solve_left(a, m, n, b, m, k)
    assert ok == consistent
    ra, rb = A.raw_bits(), B.raw_bits()
    c0 = census(L)
    rc = L.mzd_solve_left(A.ptr, B.ptr, 0, check)
    c1 = census(L)
    assert_route(c0, c1, ["gf2_elim_"])
    _outside_unchanged(A, ra)
    _outside_unchanged(B, rb)
    if consistent:
        assert rc == 0
        x = B.bits()
        assert np.array_equal(g.o_mul_m4rm(a, x, m, n, k), b), "A X != B"
    elif check:
        assert rc != 0
    A.free()
    B.free()
