"""CPU tests of the argument and aliasing contract of the device-resident API (include/m4ri_hip.h section 2): every entry checks its
arguments before a device is required and before the first HIP call, so a refused call fails the same way with and without a device --
this runs without one.  The matrices are DMatStructs around an address that is never dereferenced.

TABLE holds the rows of the header's table verbatim.  For every row of its "refused" column the call is made with the written matrix
placed on the other one in five ways (PLACEMENTS); the "allowed" rows are asserted here only where there is no device (the call is
then refused by the device check, which is the last one, and not for overlap) and run for real in tests/test_gpu_dev_aliasing.py."""
import ctypes
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "m4ri_hip.h")

# the table of include/m4ri_hip.h, row for row
TABLE = [
    '| `gf2_mul_dev`, `gf2_mul_nt_dev` | A is B / Bt; A and B overlapping; C, A, B three disjoint column ranges of one parent | C sharing a word with A or B (with or without `accumulate`) |',
    '| `gf2_add_dev` | C identical to A, to B, or to both (same `data`, `ld`, shape); A is B | C sharing a word with A or B in any other way (shifted by a row, a word, another `ld`) |',
    '| `gf2_transpose_dev` | D and S disjoint column ranges of one parent | D sharing a word with S, the square "in place" case included |',
    '| `gf2_equal_dev` | anything; A is B gives `*equal = 1` | – |',
    '| `gf2_inverse_dev` | Ainv identical to A, or overlapping it in any way (A is copied out before Ainv is written; say so) | – |',
    '| `gf2_trsm_dev` | – | B sharing a word with T |',
    '| `gf2_solve_left_dev`, `gf2_pluq_solve_left_dev` | – | B sharing a word with A |',
]
# entries with two or more matrix arguments whose rule is stated at their own declaration, and the word that states it there
OWN_RULE = {
    "gf2_copy_block_dev": "overlapping rectangles",
    "gf2_submatrix_dev": "overlapping rectangles",
    "gf2_concat_dev": "C may alias neither A nor B",
    "gf2_stack_dev": "overlapping rectangles",
    "gf2_inverse_batch_dev": "address\n * range meets A's",
    "gf2_nullspace_dev": "K cannot alias A",
}


def table_entries():
    out = {}
    for row in TABLE:
        cells = [c.strip() for c in row.strip("|").split("|")]
        assert len(cells) == 3, row
        for name in re.findall(r"`(gf2_\w+)`", cells[0]):
            out[name] = (cells[1], cells[2])
    return out


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    return p


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


BASE = 1 << 20   # an address that is never dereferenced: every call below is refused, or returns, before the first HIP call
FAR = 1 << 28    # a second buffer, far from the first
ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731


def width(ncols):
    return (ncols + 63) // 64


def mat(pkg, nrows, ncols, data=BASE, ld=None):
    s = pkg._lib.DMatStruct()
    s.data, s.ld, s.nrows, s.ncols = data, ld if ld is not None else (width(ncols) + 1) & ~1, nrows, ncols
    return s


def refused(L, rc, *words):
    msg = L.gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in words), msg


def no_device(L):
    return L.gf2_device_count() <= 0


def reaches_the_device_check(L, rc):
    """an allowed call, made only where there is no device: the one refusal left is the device check, which comes last"""
    msg = L.gf2_last_error().decode()
    assert rc != 0 and "no usable HIP device" in msg and "overlap" not in msg, (rc, msg)


# The written matrix W (wr x wc, stride ld of its own unless "another ld") placed on the matrix R (rr rows at BASE, stride rld) so that
# the two share a word: (name, data, ld) of W.
def placements(rr, rld, wr, wc):
    ww = width(wc)
    out = [("one row in", BASE + 8 * rld, rld), ("one word in", BASE + 8, rld),
           ("the same base, another ld", BASE, rld + 2), ("its last row is the other's first", BASE - 8 * rld * (wr - 1), rld),
           ("its last word is the other's first", BASE - 8 * (ww - 1), rld)]
    return out if wr > 1 else [p for p in out if p[0] != "its last row is the other's first"] + [("a single row", BASE, rld)]


def identical(rld):
    return ("the identical view", BASE, rld)


# ---- the products ---------------------------------------------------------------------------------------------------------------------

M_, L_, N_ = 10, 100, 100   # C is 10 x 100, A 10 x 100, B / Bt 100 x 100: two words per row


def mul_call(L, name, C, A, B, accumulate=0, algo=0):
    if name == "gf2_mul_dev":
        return L.gf2_mul_dev(ref(C), ref(A), ref(B), accumulate, algo, 0, None)
    return L.gf2_mul_nt_dev(ref(C), ref(A), ref(B), accumulate, None)


@pytest.mark.parametrize("name", ["gf2_mul_dev", "gf2_mul_nt_dev"])
def test_products_refuse_a_destination_on_an_operand(pkg, L, name):
    for accumulate in (0, 1):
        for algo in ((0, 1, 2, 3) if name == "gf2_mul_dev" else (0,)):
            for what, data, ld in [identical(2)] + placements(M_, 2, M_, N_):      # C on A
                C, A, B = mat(pkg, M_, N_, data, ld), mat(pkg, M_, L_, BASE, 2), mat(pkg, L_, N_, FAR, 2)
                refused(L, mul_call(L, name, C, A, B, accumulate, algo), name, "overlap", "C and A")
            for what, data, ld in [identical(2)] + placements(L_, 2, M_, N_):      # C on B: its first rows, and rows inside it
                C, A, B = mat(pkg, M_, N_, data, ld), mat(pkg, M_, L_, FAR, 2), mat(pkg, L_, N_, BASE, 2)
                refused(L, mul_call(L, name, C, A, B, accumulate, algo), name, "overlap", "C and B")
            C = mat(pkg, M_, N_, BASE + 8 * 2 * 50, 2)
            refused(L, mul_call(L, name, C, mat(pkg, M_, L_, FAR, 2), mat(pkg, L_, N_, BASE, 2), accumulate, algo), "overlap")
    # one parent of 8 words per row: C in words 0-1, A in words 2-3, B in words 1-2 meets both
    C, A = mat(pkg, M_, N_, BASE, 8), mat(pkg, M_, L_, BASE + 16, 8)
    refused(L, mul_call(L, name, C, A, mat(pkg, L_, N_, BASE + 8, 8)), "overlap", "C and B")


@pytest.mark.parametrize("name", ["gf2_mul_dev", "gf2_mul_nt_dev"])
def test_products_argument_errors(pkg, L, name):
    good = lambda: (mat(pkg, M_, N_, FAR), mat(pkg, M_, L_, BASE), mat(pkg, L_, N_, BASE + (1 << 16)))  # noqa: E731
    C, A, B = good()
    bname = "B" if name == "gf2_mul_dev" else "Bt"
    refused(L, mul_call(L, name, None, A, B), name, "C is null")
    refused(L, mul_call(L, name, C, None, B), name, "A is null")
    refused(L, mul_call(L, name, C, A, None), name, bname + " is null")
    refused(L, mul_call(L, name, mat(pkg, M_, N_, None), A, B), name, "C.data is null")
    refused(L, mul_call(L, name, C, mat(pkg, M_, L_, None), B), name, "A.data is null")
    refused(L, mul_call(L, name, C, A, mat(pkg, L_, N_, None)), name, bname + ".data is null")
    refused(L, mul_call(L, name, mat(pkg, -1, N_, FAR), A, B), name, "negative")
    refused(L, mul_call(L, name, C, mat(pkg, M_, -L_), B), name, "negative")
    refused(L, mul_call(L, name, mat(pkg, M_, N_, FAR, ld=1), A, B), name, "C.ld is smaller")
    refused(L, mul_call(L, name, C, mat(pkg, M_, L_, ld=1), B), name, "A.ld is smaller")
    refused(L, mul_call(L, name, C, A, mat(pkg, L_, N_, BASE + (1 << 16), ld=0)), name, bname + ".ld is smaller")
    refused(L, mul_call(L, name, mat(pkg, M_, N_, FAR + 4), A, B), name, "C.data is not 8-byte aligned")
    refused(L, mul_call(L, name, C, mat(pkg, M_, L_, BASE + 1), B), name, "A.data is not 8-byte aligned")
    refused(L, mul_call(L, name, mat(pkg, M_ + 1, N_, FAR), A, B), name, "dimension mismatch")
    refused(L, mul_call(L, name, mat(pkg, M_, N_ + 1, FAR), A, B), name, "dimension mismatch")
    refused(L, mul_call(L, name, C, mat(pkg, M_, L_ + 1), B), name, "dimension mismatch")


@pytest.mark.parametrize("name", ["gf2_mul_dev", "gf2_mul_nt_dev"])
def test_an_empty_product_is_no_error_and_needs_no_device(pkg, L, name):
    for m, n in ((0, 7), (7, 0), (0, 0)):
        bshape = (5, n) if name == "gf2_mul_dev" else (n, 5)
        assert mul_call(L, name, mat(pkg, m, n, None), mat(pkg, m, 5, None if m == 0 else BASE), mat(pkg, *bshape, None if n == 0 else FAR)) == 0
    # empty and on top of each other: nothing is written, nothing is refused
    assert mul_call(L, name, mat(pkg, 0, 100), mat(pkg, 0, 100), mat(pkg, 100, 100)) == 0


@pytest.mark.parametrize("name", ["gf2_mul_dev", "gf2_mul_nt_dev"])
def test_products_allowed_aliasing_is_not_refused(pkg, L, name):
    if not no_device(L):
        return  # with a device these calls would run: tests/test_gpu_dev_aliasing.py runs them
    n = 100
    A = mat(pkg, n, n, BASE, 2)
    reaches_the_device_check(L, mul_call(L, name, mat(pkg, n, n, FAR, 2), A, A))                                   # A is B / Bt
    reaches_the_device_check(L, mul_call(L, name, mat(pkg, n, n, FAR, 2), A, mat(pkg, n, n, BASE + 16 * 7, 2)))    # A and B overlapping
    # C, A, B three disjoint column ranges of one parent of 6 words per row
    reaches_the_device_check(L, mul_call(L, name, mat(pkg, n, n, BASE, 6), mat(pkg, n, n, BASE + 16, 6), mat(pkg, n, n, BASE + 32, 6)))


# ---- gf2_add_dev ------------------------------------------------------------------------------------------------------------------------

def test_add_refuses_every_overlap_but_the_identical_view(pkg, L):
    r, c = 10, 200   # four words per row
    for what, data, ld in placements(r, 4, r, c):
        W = mat(pkg, r, c, data, ld)
        refused(L, L.gf2_add_dev(ref(W), ref(mat(pkg, r, c, BASE, 4)), ref(mat(pkg, r, c, FAR, 4)), None), "gf2_add_dev", "overlap", "C and A")
        refused(L, L.gf2_add_dev(ref(W), ref(mat(pkg, r, c, FAR, 4)), ref(mat(pkg, r, c, BASE, 4)), None), "gf2_add_dev", "overlap", "C and B")
        # C identical to A does not excuse its overlap with B, and the other way round
        refused(L, L.gf2_add_dev(ref(W), ref(W), ref(mat(pkg, r, c, BASE, 4)), None), "overlap", "C and B")
        refused(L, L.gf2_add_dev(ref(W), ref(mat(pkg, r, c, BASE, 4)), ref(W), None), "overlap", "C and A")
    # the same base and ld, but another shape, is not the identical view -- such a call is a shape mismatch before it is an overlap
    refused(L, L.gf2_add_dev(ref(mat(pkg, r, c)), ref(mat(pkg, r, c - 1)), ref(mat(pkg, r, c, FAR)), None), "dimension mismatch")


def test_add_in_place_is_not_refused(pkg, L):
    if not no_device(L):
        return
    A, B = mat(pkg, 10, 200, BASE, 4), mat(pkg, 10, 200, FAR, 4)
    A2 = mat(pkg, 10, 200, BASE, 4)   # the same view in a second struct
    for C, X, Y in ((A, A, B), (A, B, A), (A, A, A), (A2, A, B), (A2, A, A2), (B, A, A),
                    (mat(pkg, 10, 200, BASE, 12), mat(pkg, 10, 200, BASE + 32, 12), mat(pkg, 10, 200, BASE + 64, 12))):
        reaches_the_device_check(L, L.gf2_add_dev(ref(C), ref(X), ref(Y), None))


def test_add_argument_errors_and_empty_shapes(pkg, L):
    C, A, B = mat(pkg, 10, 200, FAR), mat(pkg, 10, 200, BASE), mat(pkg, 10, 200, BASE + (1 << 16))
    add = lambda c, a, b: L.gf2_add_dev(ref(c), ref(a), ref(b), None)  # noqa: E731
    refused(L, add(None, A, B), "gf2_add_dev", "C is null")
    refused(L, add(C, None, B), "gf2_add_dev", "A is null")
    refused(L, add(C, A, None), "gf2_add_dev", "B is null")
    refused(L, add(mat(pkg, 10, 200, None), A, B), "C.data is null")
    refused(L, add(C, A, mat(pkg, 10, 200, None)), "B.data is null")
    refused(L, add(C, mat(pkg, 10, -200), B), "negative")
    refused(L, add(C, mat(pkg, 10, 200, ld=3), B), "A.ld is smaller")
    refused(L, add(mat(pkg, 10, 200, FAR, ld=3), A, B), "C.ld is smaller")
    refused(L, add(C, A, mat(pkg, 10, 200, BASE + (1 << 16) + 2)), "B.data is not 8-byte aligned")
    refused(L, add(C, A, mat(pkg, 11, 200, BASE + (1 << 16))), "dimension mismatch")
    refused(L, add(mat(pkg, 10, 201, FAR), A, B), "dimension mismatch")
    for r, c in ((0, 200), (10, 0), (0, 0)):
        assert add(mat(pkg, r, c, None), mat(pkg, r, c, None), mat(pkg, r, c, None)) == 0


# ---- gf2_transpose_dev ------------------------------------------------------------------------------------------------------------------

def test_transpose_refuses_a_destination_on_its_source(pkg, L):
    tr = lambda d, s: L.gf2_transpose_dev(ref(d), ref(s), None)  # noqa: E731
    n = 130   # square, three words per row: "in place"
    for what, data, ld in [identical(4)] + placements(n, 4, n, n):
        refused(L, tr(mat(pkg, n, n, data, ld), mat(pkg, n, n, BASE, 4)), "gf2_transpose_dev", "overlap", "D and S")
    r, c = 70, 130   # S is 70 x 130 (3 words), D 130 x 70 (2 words)
    for what, data, ld in placements(r, 4, c, r):
        refused(L, tr(mat(pkg, c, r, data, ld), mat(pkg, r, c, BASE, 4)), "gf2_transpose_dev", "overlap")
    if no_device(L):  # D and S disjoint column ranges of one parent of 6 words per row
        reaches_the_device_check(L, tr(mat(pkg, c, r, BASE + 24, 6), mat(pkg, r, c, BASE, 6)))


def test_transpose_argument_errors_and_empty_shapes(pkg, L):
    tr = lambda d, s: L.gf2_transpose_dev(ref(d), ref(s), None)  # noqa: E731
    S, D = mat(pkg, 70, 130), mat(pkg, 130, 70, FAR)
    refused(L, tr(None, S), "gf2_transpose_dev", "D is null")
    refused(L, tr(D, None), "gf2_transpose_dev", "S is null")
    refused(L, tr(mat(pkg, 130, 70, None), S), "D.data is null")
    refused(L, tr(D, mat(pkg, 70, 130, None)), "S.data is null")
    refused(L, tr(D, mat(pkg, -70, 130)), "negative")
    refused(L, tr(D, mat(pkg, 70, 130, ld=2)), "S.ld is smaller")
    refused(L, tr(mat(pkg, 130, 70, FAR, ld=1), S), "D.ld is smaller")
    refused(L, tr(mat(pkg, 130, 70, FAR + 4), S), "D.data is not 8-byte aligned")
    refused(L, tr(mat(pkg, 70, 130, FAR), S), "dimension mismatch")
    refused(L, tr(mat(pkg, 130, 71, FAR), S), "dimension mismatch")
    for r, c in ((0, 130), (70, 0), (0, 0)):
        assert tr(mat(pkg, c, r, None), mat(pkg, r, c, None)) == 0


# ---- gf2_equal_dev ----------------------------------------------------------------------------------------------------------------------

def test_equal_argument_errors_empty_shapes_and_aliasing(pkg, L):
    out = ctypes.c_int(7)
    eq = lambda a, b, o=out: L.gf2_equal_dev(ref(a), ref(b), ref(o) if o is not None else None, None)  # noqa: E731
    A, B = mat(pkg, 10, 200), mat(pkg, 10, 200, FAR)
    refused(L, eq(None, B), "gf2_equal_dev", "A is null")
    refused(L, eq(A, None), "gf2_equal_dev", "B is null")
    refused(L, eq(A, B, None), "gf2_equal_dev", "equal is null")
    refused(L, eq(mat(pkg, 10, 200, None), B), "A.data is null")
    refused(L, eq(A, mat(pkg, 10, -200, FAR)), "negative")
    refused(L, eq(A, mat(pkg, 10, 200, FAR, ld=3)), "B.ld is smaller")
    refused(L, eq(mat(pkg, 10, 200, BASE + 4), B), "A.data is not 8-byte aligned")
    assert out.value == 7   # a refused call does not write through `equal`
    assert eq(A, mat(pkg, 10, 201, FAR)) == 0 and out.value == 0   # another shape: not equal, no device needed (mzd_equal)
    out.value = 7
    assert eq(mat(pkg, 0, 200, None), mat(pkg, 0, 200, None)) == 0 and out.value == 1
    if no_device(L):  # nothing is written: any aliasing reaches the device check
        for X in (A, mat(pkg, 10, 200, BASE + 8), mat(pkg, 10, 200, BASE, ld=6)):
            reaches_the_device_check(L, eq(A, X))


# ---- gf2_inverse_dev --------------------------------------------------------------------------------------------------------------------

def test_inverse_argument_errors_empty_shapes_and_aliasing(pkg, L):
    sing = ctypes.c_int(7)
    inv = lambda i, a, s=sing: L.gf2_inverse_dev(ref(i), ref(a), ref(s) if s is not None else None, None)  # noqa: E731
    n = 130
    A, Ai = mat(pkg, n, n), mat(pkg, n, n, FAR)
    refused(L, inv(None, A), "gf2_inverse_dev", "Ainv is null")
    refused(L, inv(Ai, None), "gf2_inverse_dev", "A is null")
    refused(L, inv(Ai, A, None), "gf2_inverse_dev", "singular is null")
    refused(L, inv(mat(pkg, n, n, None), A), "Ainv.data is null")
    refused(L, inv(Ai, mat(pkg, n, n, None)), "A.data is null")
    refused(L, inv(Ai, mat(pkg, -n, -n)), "negative")
    refused(L, inv(Ai, mat(pkg, n, n, ld=2)), "A.ld is smaller")          # the check the entry did not have
    refused(L, inv(mat(pkg, n, n, FAR, ld=2), A), "Ainv.ld is smaller")
    refused(L, inv(mat(pkg, n, n, FAR + 4), A), "Ainv.data is not 8-byte aligned")
    refused(L, inv(Ai, mat(pkg, n, n + 1)), "square")
    refused(L, inv(mat(pkg, n + 1, n + 1, FAR), A), "square")
    assert sing.value == 7
    assert inv(mat(pkg, 0, 0, None), mat(pkg, 0, 0, None)) == 0 and sing.value == 0
    if no_device(L):  # Ainv identical to A, or overlapping it in any way
        for what, data, ld in [identical(4)] + placements(n, 4, n, n):
            reaches_the_device_check(L, inv(mat(pkg, n, n, data, ld), mat(pkg, n, n, BASE, 4)))


# ---- gf2_trsm_dev -----------------------------------------------------------------------------------------------------------------------

def test_trsm_refuses_a_right_hand_side_on_the_triangle(pkg, L):
    n, k = 130, 200
    for right in (0, 1):
        br, bc = (k, n) if right else (n, k)
        for upper in (0, 1):
            for what, data, ld in [identical(4)] + placements(n, 4, br, bc):
                refused(L, L.gf2_trsm_dev(ref(mat(pkg, n, n, BASE, 4)), ref(mat(pkg, br, bc, data, ld)), upper, right, None),
                        "gf2_trsm_dev", "overlap", "B and T")
    refused(L, L.gf2_trsm_dev(ref(mat(pkg, n, n, BASE, 4)), ref(mat(pkg, n, n, BASE, 4)), 0, 0, None), "overlap")   # B is T
    if no_device(L):  # two column ranges of one parent
        reaches_the_device_check(L, L.gf2_trsm_dev(ref(mat(pkg, n, n, BASE, 8)), ref(mat(pkg, n, k, BASE + 24, 8)), 0, 0, None))


def test_trsm_argument_errors_and_empty_shapes(pkg, L):
    n, k = 130, 200
    trsm = lambda t, b, right=0: L.gf2_trsm_dev(ref(t), ref(b), 0, right, None)  # noqa: E731
    T, B = mat(pkg, n, n), mat(pkg, n, k, FAR)
    refused(L, trsm(None, B), "gf2_trsm_dev", "T is null")
    refused(L, trsm(T, None), "gf2_trsm_dev", "B is null")
    refused(L, trsm(mat(pkg, n, n, None), B), "T.data is null")
    refused(L, trsm(T, mat(pkg, n, k, None)), "B.data is null")
    refused(L, trsm(T, mat(pkg, n, -k, FAR)), "negative")
    refused(L, trsm(mat(pkg, n, n, ld=2), B), "T.ld is smaller")
    refused(L, trsm(T, mat(pkg, n, k, FAR, ld=3)), "B.ld is smaller")
    refused(L, trsm(T, mat(pkg, n, k, FAR + 4)), "B.data is not 8-byte aligned")
    refused(L, trsm(mat(pkg, n, n + 1), B), "not square")
    refused(L, trsm(T, mat(pkg, n + 1, k, FAR)), "dimension mismatch")
    refused(L, trsm(T, B, right=1), "dimension mismatch")
    assert trsm(mat(pkg, 0, 0, None), mat(pkg, 0, k, None)) == 0
    assert trsm(T, mat(pkg, n, 0, None)) == 0
    assert trsm(T, mat(pkg, 0, n, None), right=1) == 0


# ---- gf2_solve_left_dev, gf2_pluq_solve_left_dev ----------------------------------------------------------------------------------------

def solve_call(L, name, A, B, bad, rank=0):
    if name == "gf2_solve_left_dev":
        return L.gf2_solve_left_dev(ref(A), ref(B), 1, ref(bad) if bad is not None else None, None)
    m, n = (A.nrows, A.ncols) if A is not None else (1, 1)
    P, Q = (ctypes.c_int * max(m, 1))(*range(max(m, 0))), (ctypes.c_int * max(n, 1))(*range(max(n, 0)))
    return L.gf2_pluq_solve_left_dev(ref(A), rank, P, Q, ref(B), 1, ref(bad) if bad is not None else None, None)


@pytest.mark.parametrize("name", ["gf2_solve_left_dev", "gf2_pluq_solve_left_dev"])
def test_solves_refuse_a_right_hand_side_on_the_matrix(pkg, L, name):
    m, n, k = 100, 130, 200   # A is 100 x 130 (3 words), B 130 x 200 (4 words)
    bad = ctypes.c_int(7)
    for what, data, ld in [identical(4)] + placements(m, 4, n, k):
        refused(L, solve_call(L, name, mat(pkg, m, n, BASE, 4), mat(pkg, n, k, data, ld), bad), name, "overlap", "B and A")
    refused(L, solve_call(L, name, mat(pkg, n, n, BASE, 4), mat(pkg, n, n, BASE, 4), bad), name, "overlap")   # B is A
    if no_device(L):  # two column ranges of one parent
        reaches_the_device_check(L, solve_call(L, name, mat(pkg, m, n, BASE, 8), mat(pkg, n, k, BASE + 24, 8), bad))


@pytest.mark.parametrize("name", ["gf2_solve_left_dev", "gf2_pluq_solve_left_dev"])
def test_solves_argument_errors_and_empty_shapes(pkg, L, name):
    m, n, k = 100, 130, 200
    bad = ctypes.c_int(7)
    A, B = mat(pkg, m, n), mat(pkg, n, k, FAR)
    refused(L, solve_call(L, name, None, B, bad), name, "null")
    refused(L, solve_call(L, name, A, None, bad), name, "null")
    refused(L, solve_call(L, name, A, B, None), name, "null", "inconsistent")
    refused(L, solve_call(L, name, mat(pkg, m, n, None), B, bad), name, "null")
    refused(L, solve_call(L, name, A, mat(pkg, n, k, None), bad), name, "null")
    refused(L, solve_call(L, name, A, mat(pkg, n, -k, FAR), bad), name, "negative")
    refused(L, solve_call(L, name, mat(pkg, m, n, ld=2), B, bad), name, "smaller")
    refused(L, solve_call(L, name, A, mat(pkg, n, k, FAR, ld=3), bad), name, "smaller")
    refused(L, solve_call(L, name, A, mat(pkg, n, k, FAR + 4), bad), name, "8-byte aligned")
    refused(L, solve_call(L, name, A, mat(pkg, n - 1, k, FAR), bad), name, "B")          # B needs max(m, n) rows
    refused(L, solve_call(L, name, mat(pkg, n + 1, n), B, bad), name, "B")
    if name == "gf2_pluq_solve_left_dev":
        refused(L, solve_call(L, name, A, B, bad, rank=m + 1), name, "rank")
        refused(L, L.gf2_pluq_solve_left_dev(ref(A), 0, None, None, ref(B), 1, ref(bad), None), name, "P or Q is null")
    for a, b in ((mat(pkg, 0, n, None), B), (mat(pkg, m, 0, None), mat(pkg, m, k, FAR)), (A, mat(pkg, n, 0, None))):
        bad.value = 7
        assert solve_call(L, name, a, b, bad) == 0 and bad.value == 0


# ---- the single-matrix entries of the elimination family ----------------------------------------------------------------------------------

def test_single_matrix_entries_check_before_the_device(pkg, L):
    rank = ctypes.c_int(7)
    n = 130
    A = mat(pkg, n, n)
    P = (ctypes.c_int * n)(*range(n))
    calls = {
        "gf2_echelonize_dev": lambda a, r=rank: L.gf2_echelonize_dev(ref(a), 1, 0, ref(r) if r is not None else None, None, None),
        "gf2_ple_dev": lambda a, r=rank: L.gf2_ple_dev(ref(a), 0, P, P, ref(r) if r is not None else None, None),
        "gf2_nullspace_dev": lambda a, r=rank: L.gf2_nullspace_dev(ref(a), ref(pkg._lib.DMatStruct()), ref(r) if r is not None else None, None, None),
        "gf2_apply_p_dev": lambda a, r=rank: L.gf2_apply_p_dev(ref(a), P, n, 0, 0, None),
    }
    for name, call in calls.items():
        rank.value = 7
        refused(L, call(None), name, "A is null")
        refused(L, call(mat(pkg, n, n, None)), name, "A.data is null")
        refused(L, call(mat(pkg, -n, n)), name, "negative")
        refused(L, call(mat(pkg, n, n, ld=2)), name, "A.ld is smaller")
        refused(L, call(mat(pkg, n, n, BASE + 4)), name, "A.data is not 8-byte aligned")
        if name != "gf2_apply_p_dev":
            refused(L, call(A, None), name, "rank is null")
        assert rank.value == 7, name
        if no_device(L):
            reaches_the_device_check(L, call(A))
    refused(L, L.gf2_nullspace_dev(ref(A), None, ref(rank), None, None), "gf2_nullspace_dev", "K is null")
    refused(L, L.gf2_ple_dev(ref(A), 0, None, P, ref(rank), None), "gf2_ple_dev", "P or Q is null")
    refused(L, L.gf2_apply_p_dev(ref(A), None, n, 0, 0, None), "gf2_apply_p_dev", "P is null")
    refused(L, L.gf2_apply_p_dev(ref(A), P, -1, 0, 0, None), "gf2_apply_p_dev", "len is negative")
    P[3] = n
    refused(L, L.gf2_apply_p_dev(ref(A), P, n, 0, 0, None), "gf2_apply_p_dev", "out of range")
    P[3] = 3
    # empty shapes: 0 without a device
    for r, c in ((0, n), (n, 0)):
        rank.value = 7
        assert calls["gf2_echelonize_dev"](mat(pkg, r, c, None)) == 0 and rank.value == 0
        rank.value = 7
        assert calls["gf2_ple_dev"](mat(pkg, r, c, None)) == 0 and rank.value == 0
        assert L.gf2_apply_p_dev(ref(mat(pkg, r, c, None)), P, 0, 0, 0, None) == 0
    K = pkg._lib.DMatStruct()
    rank.value = 7
    assert L.gf2_nullspace_dev(ref(mat(pkg, n, 0, None)), ref(K), ref(rank), None, None) == 0 and rank.value == 0 and not K.data


# ---- the predicate against brute force -------------------------------------------------------------------------------------------------

def test_share_a_word_against_the_word_sets(pkg, L):
    """"Share a word" on random small views of one buffer, through gf2_transpose_dev(D, S): with one ld the refusal is exact -- the two
    sets of word addresses meet --, with two it is the intersection of the address ranges.  A call that is expected to pass is made
    only where there is no device (it ends at the device check); with a device only the refusals are made."""
    import random
    rng = random.Random(20260101)
    words = lambda base, ld, rows, cols: {base + i * ld + j for i in range(rows) for j in range(width(cols))}  # noqa: E731
    seen = {True: 0, False: 0}
    for _ in range(4000):
        r, c = rng.randint(1, 6), rng.randint(1, 200)
        lds = rng.randint(width(c), width(c) + 4)
        ldd = lds if rng.random() < 0.7 else rng.randint(width(r), width(r) + 4)
        if ldd < width(r):
            continue
        s0, d0 = rng.randint(0, 40), rng.randint(0, 40)
        ws, wd = words(s0, lds, r, c), words(d0, ldd, c, r)
        expect = bool(ws & wd) if lds == ldd else (min(ws) <= max(wd) and min(wd) <= max(ws))
        seen[expect] += 1
        if not expect and not no_device(L):
            continue
        rc = L.gf2_transpose_dev(ref(mat(pkg, c, r, BASE + 8 * d0, ldd)), ref(mat(pkg, r, c, BASE + 8 * s0, lds)), None)
        if expect:
            refused(L, rc, "overlap")
        else:
            reaches_the_device_check(L, rc)
    assert min(seen.values()) > 300, seen


# ---- the table and the header ---------------------------------------------------------------------------------------------------------------

def section2():
    text = open(HEADER).read()
    return text[text.index("2. Device-resident API"):]


def entries_with_two_matrices(text):
    """every function of section 2 whose declaration names gf2_dmat twice or more"""
    out = []
    for m in re.finditer(r"^\w[\w \*]*?\b(gf2_\w+)\s*\(([^;{]*)\)\s*;", text, re.M):
        if len(re.findall(r"\bgf2_dmat\b", m.group(2))) >= 2:
            out.append(m.group(1))
    return out


def test_the_table_is_in_the_header_row_for_row():
    text = section2()
    for row in TABLE:
        assert " * " + row + "\n" in text, row
    assert "| entry | allowed aliasing | refused (-1, \"overlap\") |" in text


def test_every_entry_with_two_matrices_has_a_stated_rule():
    text = section2()
    found = entries_with_two_matrices(text)
    stated = table_entries()
    # the parser sees what it should: these take two or three matrices ...
    for name in ("gf2_mul_dev", "gf2_add_dev", "gf2_transpose_dev", "gf2_trsm_dev", "gf2_pluq_solve_left_dev", "gf2_concat_dev",
                 "gf2_inverse_batch_dev", "gf2_nullspace_dev"):
        assert name in found, (name, found)
    # ... and these one
    for name in ("gf2_echelonize_dev", "gf2_ple_dev", "gf2_dmat_upload", "gf2_echelonize_batch_dev"):
        assert name not in found, name
    for name in found:
        assert name in stated or name in OWN_RULE, "%s takes two or more matrices and has no row in the aliasing table" % name
    for name, words in OWN_RULE.items():
        assert name in found and words in text, name
    assert sorted(stated) == sorted(n for n in found if n not in OWN_RULE)


def test_the_parser_notices_an_entry_without_a_row():
    text = section2() + "\nint gf2_kron_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream);\n"
    missing = [n for n in entries_with_two_matrices(text) if n not in table_entries() and n not in OWN_RULE]
    assert missing == ["gf2_kron_dev"]


def test_every_refused_column_has_a_test():
    """the rows with a refusal are the ones the refusal tests above call"""
    refusing = sorted(n for n, (_, refusedcol) in table_entries().items() if refusedcol != "–")
    assert refusing == ["gf2_add_dev", "gf2_mul_dev", "gf2_mul_nt_dev", "gf2_pluq_solve_left_dev", "gf2_solve_left_dev",
                        "gf2_transpose_dev", "gf2_trsm_dev"]
