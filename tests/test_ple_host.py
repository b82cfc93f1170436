"""CPU tests of mzp_t, the mzd_apply_p_* family, and mzd_ple / mzd_pluq / mzd_pluq_solve_left through the host routine of the
size dispatch (M4RI_HIP_HOST_SMALL_WORK), against the pure-Python model tests/ple_ref.py and the committed fixtures
tests/golden/ple/*.npz.  No device is needed."""
import ctypes
import glob
import os
import random

import numpy as np
import pytest

import gf2util as g
import ple_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device  # noqa: F401  (p.device.Mzp)
    return p


@pytest.fixture
def host_small(monkeypatch):
    monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", str(1 << 40))


def mzp(pkg, values):
    from m4ri_rust_amd import device
    return device.Mzp.from_list(values)


def rand_perm(n, rng):
    return [rng.randrange(i, n) for i in range(n)]


def dirty_window(pkg, rows, cols, seed, r0=3, c0=64, extra=70):
    """(parent BinMatrix, window mzd_t*) with random bits in every parent word, excess bits included"""
    pc = c0 + cols + extra
    P = pkg.BinMatrix.from_words(g.random_words(r0 + rows + 2, pc, seed), pc)
    w = g.width(pc)
    P._words_view()[:, :w] = g.splitmix64(seed ^ 0x5EED, np.arange((r0 + rows + 2) * w, dtype=np.uint64)).reshape(-1, w)
    W = pkg._lib.lib().mzd_init_window(P.mzd, r0, c0, r0 + rows, c0 + cols)
    return P, W


def window_rows(P, r0, c0, rows, cols):
    b = g.words_to_bits(P.to_words(), P.ncols())
    return R.rows_of(g.bits_to_words(b[r0:r0 + rows, c0:c0 + cols]), cols)


def test_mzp_basics(pkg, capfd):
    L = pkg._lib.lib()
    p = L.mzp_init(7)
    assert [p.contents.values[i] for i in range(7)] == list(range(7)) and p.contents.length == 7
    for i, v in enumerate([3, 1, 4, 4, 6, 5, 6]):
        p.contents.values[i] = v
    c = L.mzp_copy(None, p)
    assert [c.contents.values[i] for i in range(7)] == [3, 1, 4, 4, 6, 5, 6]
    d = L.mzp_init(9)
    assert L.mzp_copy(d, p)
    assert [d.contents.values[i] for i in range(9)] == [3, 1, 4, 4, 6, 5, 6, 7, 8]
    w = L.mzp_init_window(p, 2, 5)
    assert w.contents.length == 3 and [w.contents.values[i] for i in range(3)] == [4, 4, 6]
    w.contents.values[0] = 2  # the window's values are the parent's
    assert p.contents.values[2] == 2
    L.Mzp_free_window(w)
    w2 = L.mzp_init_window(p, 0, 7)
    L.mzp_free_window(w2)
    L.mzp_print(p)
    out = capfd.readouterr().out
    assert out.strip() == "[3 1 2 4 6 5 6]"
    L.mzp_set_ui(p, 1)
    assert [p.contents.values[i] for i in range(7)] == list(range(7))
    for x in (p, c, d):
        L.mzp_free(x)


def test_mzp_free_window_exported(pkg):
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], text=True)
    names = {ln.split()[-1] for ln in out.splitlines()}
    for n in ("Mzp_free_window", "mzp_free_window", "mzp_init", "mzp_free", "mzp_copy", "mzp_init_window", "mzp_set_ui",
              "mzp_print", "mzd_apply_p_left", "mzd_apply_p_left_trans", "mzd_apply_p_right", "mzd_apply_p_right_trans",
              "mzd_ple", "mzd_pluq", "mzd_pluq_solve_left", "gf2_ple_dev", "gf2_apply_p_dev", "gf2_pluq_solve_left_dev"):
        assert n in names, n


def test_mzp_set_ui_other_values_abort(pkg):
    import subprocess
    import sys
    code = ("import m4ri_rust_amd as p; L = p._lib.lib(); q = L.mzp_init(3); L.mzp_set_ui(q, 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True)
    assert r.returncode != 0 and "mzp_set_ui" in r.stderr


@pytest.mark.parametrize("m,n", [(1, 1), (5, 9), (64, 64), (70, 130), (130, 70)])
@pytest.mark.parametrize("window", [False, True])
def test_apply_p_against_model(pkg, m, n, window):
    L = pkg._lib.lib()
    rng = random.Random(m * 1000 + n + window)
    a = g.random_words(m, n, m + n)
    for plen_rows, plen_cols in ((m, n), (max(m - 3, 0), max(n - 5, 0)), (m + 4, n + 4)):
        P = mzp(pkg, [rng.randrange(i, max(m, i + 1)) if i < m else i for i in range(plen_rows)])
        Qp = mzp(pkg, [rng.randrange(i, max(n, i + 1)) if i < n else i for i in range(plen_cols)])
        for fn, perm, model in (
                ("mzd_apply_p_left", P, lambda r: R.apply_left(r, P.to_list())),
                ("mzd_apply_p_left_trans", P, lambda r: R.apply_left(r, P.to_list(), trans=True)),
                ("mzd_apply_p_right", Qp, lambda r: R.apply_right(r, Qp.to_list(), n)),
                ("mzd_apply_p_right_trans", Qp, lambda r: R.apply_right(r, Qp.to_list(), n, trans=True))):
            if window:
                parent, W = dirty_window(pkg, m, n, m * 7 + n)
                before = g.words_to_bits(parent.to_words(), parent.ncols())
                rows = window_rows(parent, 3, 64, m, n)
                getattr(L, fn)(W, perm.ptr)
                after = g.words_to_bits(parent.to_words(), parent.ncols())
                mask = np.ones_like(after, dtype=bool)
                mask[3:3 + m, 64:64 + n] = False
                assert np.array_equal(after[mask], before[mask]), fn + ": parent changed outside the window"
                assert window_rows(parent, 3, 64, m, n) == model(rows), fn
                L.mzd_free(W)
            else:
                M = pkg.BinMatrix.from_words(a, n)
                getattr(L, fn)(M.mzd, perm.ptr)
                assert R.rows_of(M.to_words(), n) == model(R.rows_of(a, n)), fn


@pytest.mark.parametrize("m,n", [(33, 47), (128, 200), (200, 128)])
def test_apply_p_round_trips(pkg, m, n):
    L = pkg._lib.lib()
    rng = random.Random(m + n)
    a = g.random_words(m, n, 5)
    M = pkg.BinMatrix.from_words(a, n)
    P, Q = mzp(pkg, rand_perm(m, rng)), mzp(pkg, rand_perm(n, rng))
    L.mzd_apply_p_left(M.mzd, P.ptr)
    L.mzd_apply_p_left_trans(M.mzd, P.ptr)
    assert np.array_equal(M.to_words(), a)
    L.mzd_apply_p_right(M.mzd, Q.ptr)
    L.mzd_apply_p_right_trans(M.mzd, Q.ptr)
    assert np.array_equal(M.to_words(), a)
    # right == (left_trans on A^T)^T
    L.mzd_apply_p_right(M.mzd, Q.ptr)
    T = pkg.BinMatrix.from_words(g.o_transpose(a, m, n), m)
    L.mzd_apply_p_left_trans(T.mzd, Q.ptr)
    assert np.array_equal(g.o_transpose(T.to_words(), n, m), M.to_words())


def low_rank(m, n, r, seed):
    if r == 0:
        return np.zeros((m, g.width(n)), dtype=np.uint64)
    return g.o_mul_naive(g.random_words(m, r, seed), g.random_words(r, n, seed + 1), m, r, n)


def structured(m, n):
    yield "zero", np.zeros((m, g.width(n)), dtype=np.uint64)
    k = min(m, n)
    eye = np.zeros((m, n), dtype=np.uint8)
    eye[np.arange(k), np.arange(k)] = 1
    yield "identity", g.bits_to_words(eye)
    yield "reversed identity", g.bits_to_words(eye[::-1].copy())
    base = g.random_words(max(m // 2, 1), n, 11)
    yield "duplicated rows", np.ascontiguousarray(np.vstack([base, base, base])[:m])
    lz = g.words_to_bits(g.random_words(m, n, 12), n)
    lz[:, :min(n, 70)] = 0
    yield "leading zero columns", g.bits_to_words(lz)
    yield "all rows equal", np.ascontiguousarray(np.repeat(g.random_words(1, n, 13), m, axis=0))
    one = np.zeros((m, n), dtype=np.uint8)
    one[:, n // 2] = np.arange(m) % 3 == 1
    yield "single column", g.bits_to_words(one)


def check_ple(pkg, a, m, n, pluq):
    L = pkg._lib.lib()
    M = pkg.BinMatrix.from_words(a, n)
    P, Q = pkg.device.Mzp(m), pkg.device.Mzp(n)
    r = (L.mzd_pluq if pluq else L.mzd_ple)(M.mzd, P.ptr, Q.ptr, 0)
    rank, Pr, Qr, out = R.ple(R.rows_of(a, n), n, pluq)
    assert r == rank
    assert P.to_list() == Pr
    assert Q.to_list() == Qr
    assert R.rows_of(M.to_words(), n) == out
    return r


@pytest.mark.parametrize("m,n", [(1, 1), (63, 65), (64, 64), (65, 129), (120, 300), (300, 120)])
@pytest.mark.parametrize("pluq", [False, True])
def test_ple_host_random_and_structured(pkg, host_small, m, n, pluq):
    check_ple(pkg, g.random_words(m, n, m * 3 + n), m, n, pluq)
    for r in (0, 1, 63, 64, 65):
        if r <= min(m, n):
            check_ple(pkg, low_rank(m, n, r, r + 7), m, n, pluq)
    for name, a in structured(m, n):
        check_ple(pkg, a, m, n, pluq)


def test_library_ple_identity_holds(pkg, host_small):
    """mzd_ple / mzd_pluq output of the library: P A0 = L E and P A0 Q^T = L U, with L unit lower and E / U in echelon form"""
    L = pkg._lib.lib()
    m, n = 150, 170
    a = low_rank(m, n, 90, 3)
    rows = R.rows_of(a, n)
    for pluq in (False, True):
        M = pkg.BinMatrix.from_words(a, n)
        P, Q = pkg.device.Mzp(m), pkg.device.Mzp(n)
        rank = (L.mzd_pluq if pluq else L.mzd_ple)(M.mzd, P.ptr, Q.ptr, 0)
        assert rank == 90
        out = R.rows_of(M.to_words(), n)
        Lr, U = R.split_le(out, rank, n)
        lhs = R.apply_left(rows, P.to_list())
        if pluq:
            lhs = R.apply_right(lhs, Q.to_list(), n, trans=True)
            assert all(U[i] & ((1 << (i + 1)) - 1) == 1 << i for i in range(rank)), "U is not unit upper triangular"
        else:
            assert all((U[i] & -U[i]) == 1 << Q.to_list()[i] for i in range(rank)), "E_i does not lead at Q[i]"
        assert R.mul(Lr, U) == lhs


def test_ple_rejects_wrong_lengths(pkg):
    import subprocess
    import sys
    code = ("import m4ri_rust_amd as p; from m4ri_rust_amd import device; L = p._lib.lib(); M = L.mzd_init(4, 5); "
            "P = device.Mzp(3); Q = device.Mzp(5); L.mzd_ple(M, P.ptr, Q.ptr, 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True,
                       env=dict(os.environ, M4RI_HIP_HOST_SMALL_WORK="1000000"))
    assert r.returncode != 0 and "mzd_ple" in r.stderr


def test_ple_host_on_dirty_window(pkg, host_small):
    L = pkg._lib.lib()
    m, n = 90, 150
    for pluq in (False, True):
        parent, W = dirty_window(pkg, m, n, 21)
        before = g.words_to_bits(parent.to_words(), parent.ncols())
        rows = window_rows(parent, 3, 64, m, n)
        P, Q = pkg.device.Mzp(m), pkg.device.Mzp(n)
        r = (L.mzd_pluq if pluq else L.mzd_ple)(W, P.ptr, Q.ptr, 0)
        rank, Pr, Qr, out = R.ple(rows, n, pluq)
        assert (r, P.to_list(), Q.to_list()) == (rank, Pr, Qr)
        assert window_rows(parent, 3, 64, m, n) == out
        after = g.words_to_bits(parent.to_words(), parent.ncols())
        mask = np.ones_like(after, dtype=bool)
        mask[3:3 + m, 64:64 + n] = False
        assert np.array_equal(after[mask], before[mask])
        L.mzd_free(W)


@pytest.mark.parametrize("m,n,k,r", [(40, 40, 1, 40), (60, 90, 64, 50), (90, 60, 300, 45), (100, 100, 64, 100)])
def test_pluq_solve_left_host(pkg, host_small, m, n, k, r):
    L = pkg._lib.lib()
    a = low_rank(m, n, r, m + n + k)
    x0 = g.random_words(n, k, 9)
    b = g.o_mul_naive(a, x0, m, n, k)  # consistent
    for consistent in (True, False):
        bb = b.copy() if consistent else g.random_words(m, k, 10)
        brows = max(m, n)
        B = pkg.BinMatrix.from_words(np.vstack([bb, g.random_words(brows - m, k, 4)]) if brows > m else bb, k)
        A = pkg.BinMatrix.from_words(a, n)
        P, Q = pkg.device.Mzp(m), pkg.device.Mzp(n)
        rank = L.mzd_pluq(A.mzd, P.ptr, Q.ptr, 0)
        rc = L.mzd_pluq_solve_left(A.mzd, rank, P.ptr, Q.ptr, B.mzd, 0, 1)
        x = B.to_words()
        if consistent:
            assert rc == 0
            assert np.array_equal(g.o_mul_naive(a, x[:n], m, n, k), bb)
            want, ok = R.solve_free_zero(R.rows_of(a, n), n, R.rows_of(bb, k))
            assert ok and R.rows_of(x[:n], k) == want
            assert not x[n:].any()
        elif rank < m:
            assert rc == -1


def test_golden_fixtures(pkg, host_small):
    files = sorted(glob.glob(os.path.join(HERE, "golden", "ple", "*.npz")))
    assert files
    for f in files:
        z = np.load(f)
        m, n = int(z["m"]), int(z["n"])
        for pluq, key in ((False, "ple"), (True, "pluq")):
            L = pkg._lib.lib()
            M = pkg.BinMatrix.from_words(z["a"], n)
            P, Q = pkg.device.Mzp(m), pkg.device.Mzp(n)
            r = (L.mzd_pluq if pluq else L.mzd_ple)(M.mzd, P.ptr, Q.ptr, 0)
            assert r == int(z["rank"]), f
            assert P.to_list() == z["P"].tolist() and Q.to_list() == z["Q"].tolist(), f
            assert np.array_equal(M.to_words(), z[key]), f
