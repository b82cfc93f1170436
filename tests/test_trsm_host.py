"""CPU tests of gf2_trsm_host_small, the host routine of mzd_trsm_*'s size dispatch: all four variants against the numpy
substitution, the product identity and the closed forms of tests/trsm_ref.py and the fixtures tests/golden/trsm/*.npz; T with
anything in its other triangle and on its diagonal; T and B as windows of dirty parents.  No device is needed."""
import glob
import os

import numpy as np
import pytest

import gf2util as g
import trsm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    return p


def run_host(pkg):
    L = pkg._lib.lib()

    def run(tw, bw, n, rows, cols, upper, right):
        T, B = pkg.BinMatrix.from_words(tw, n), pkg.BinMatrix.from_words(bw, cols)
        assert L.gf2_trsm_host_small(T.mzd, B.mzd, int(upper), int(right)) == 0
        assert np.array_equal(T.to_words(), tw), "T changed"
        return B.to_words()
    return run


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 300])
@pytest.mark.parametrize("k", [1, 64, 65, 200])
def test_host_small_all_variants(pkg, n, k):
    before = pkg._lib.lib().gf2_host_small_calls()
    for upper, right in R.VARIANTS:
        R.check_variant(run_host(pkg), n, k, upper, right, seed=1000 * n + k)
    assert pkg._lib.lib().gf2_host_small_calls() == before + 12  # three solves per variant


@pytest.mark.parametrize("n,k", [(2, 1), (65, 64), (129, 65), (300, 200)])
def test_dirty_t_gives_the_clean_result(pkg, n, k):
    run = run_host(pkg)
    for upper, right in R.VARIANTS:
        rows, cols = R.b_shape(n, k, right)
        tb = R.random_bits(n, n, n + k)
        b0 = g.random_words(rows, cols, n + k + 1)
        want = run(g.bits_to_words(R.clean(tb, upper)), b0.copy(), n, rows, cols, upper, right)
        for zero_diagonal in (False, True):
            td = R.dirty(tb, upper, 3 * n + k, zero_diagonal)
            assert np.array_equal(run(g.bits_to_words(td), b0.copy(), n, rows, cols, upper, right), want), R.name(upper, right)


def dirty_parent(pkg, nrows, ncols, seed):
    """random bits in every word of every row, the excess bits of the last word included"""
    P = pkg.BinMatrix.from_words(g.random_words(nrows, ncols, seed), ncols)
    w = g.width(ncols)
    P._words_view()[:, :w] = g.splitmix64(seed ^ 0x5EED, np.arange(nrows * w, dtype=np.uint64)).reshape(nrows, w)
    return P


def raw_bits(P):
    return g.words_to_bits(P.to_words(), g.width(P.ncols()) * 64)


def windows_case(pkg, call, n, k, upper, right, one_parent, seed):
    """call(T window, B window); T at (3, 64) of its parent, B at (5, 128) of its own parent or right of T in T's parent.
    Returns X; checks that nothing outside B's window changed."""
    L = pkg._lib.lib()
    rows, cols = R.b_shape(n, k, right)
    tcols = 64 * g.width(n)
    if one_parent:
        br, bc = 3, 64 + tcols + 64
        PT = PB = dirty_parent(pkg, 3 + max(n, rows) + 2, bc + cols + 70, seed)
    else:
        br, bc = 5, 128
        PT = dirty_parent(pkg, 3 + n + 2, 64 + n + 70, seed)
        PB = dirty_parent(pkg, br + rows + 1, bc + cols + 70, seed + 1)
    before_t, before_b = raw_bits(PT), raw_bits(PB)
    tb = before_t[3:3 + n, 64:64 + n]
    b0 = g.bits_to_words(before_b[br:br + rows, bc:bc + cols].copy())
    TW = L.mzd_init_window(PT.mzd, 3, 64, 3 + n, 64 + n)
    BW = L.mzd_init_window(PB.mzd, br, bc, br + rows, bc + cols)
    call(TW, BW)
    L.mzd_free(TW)
    L.mzd_free(BW)
    after_b = raw_bits(PB)
    mask = np.ones_like(after_b, dtype=bool)
    mask[br:br + rows, bc:bc + cols] = False
    assert np.array_equal(after_b[mask], before_b[mask]), "B's parent changed outside the window"
    if not one_parent:
        assert np.array_equal(raw_bits(PT), before_t), "T's parent changed"
    x = g.bits_to_words(after_b[br:br + rows, bc:bc + cols].copy())
    assert np.array_equal(x, R.solve(tb, b0, rows, cols, upper, right)), R.name(upper, right) + ": differs from the substitution"
    R.check_product(tb, x, b0, rows, cols, upper, right)
    return x


@pytest.mark.parametrize("n,k", [(63, 65), (65, 1), (129, 200), (300, 64)])
@pytest.mark.parametrize("one_parent", [False, True])
def test_windows_of_dirty_parents(pkg, n, k, one_parent):
    L = pkg._lib.lib()
    for upper, right in R.VARIANTS:
        windows_case(pkg, lambda T, B: L.gf2_trsm_host_small(T, B, int(upper), int(right)), n, k, upper, right, one_parent,
                     seed=n * 7 + k)


def test_golden_fixtures(pkg):
    files = sorted(glob.glob(os.path.join(HERE, "golden", "trsm", "*.npz")))
    assert len(files) == 3
    run = run_host(pkg)
    for f in files:
        z = np.load(f)
        n, k = int(z["n"]), int(z["k"])
        for upper, right in R.VARIANTS:
            rows, cols = R.b_shape(n, k, right)
            got = run(z["t"], z["b_right" if right else "b_left"].copy(), n, rows, cols, upper, right)
            assert np.array_equal(got, z["x_" + R.name(upper, right)]), (f, R.name(upper, right))


def test_bad_dimensions_are_refused(pkg):
    L = pkg._lib.lib()
    T, B = pkg.BinMatrix.zero(4, 5), pkg.BinMatrix.zero(4, 3)
    assert L.gf2_trsm_host_small(T.mzd, B.mzd, 0, 0) == -1  # not square
    T = pkg.BinMatrix.zero(4, 4)
    assert L.gf2_trsm_host_small(T.mzd, B.mzd, 0, 1) == -1  # X T = B needs 4 columns
    assert L.gf2_trsm_host_small(T.mzd, B.mzd, 0, 0) == 0


def test_host_entries_abort_on_bad_dimensions(pkg):
    import subprocess
    import sys
    code = ("import m4ri_rust_amd as p; L = p._lib.lib(); T = L.mzd_init(4, 5); B = L.mzd_init(4, 3); "
            "L.mzd_trsm_lower_left(T, B, 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True)
    assert r.returncode != 0 and "mzd_trsm_lower_left" in r.stderr
