"""CPU tests of the C oracle's PLE / PLUQ and transposition lists (oracle_ple, oracle_apply_p) against the pure-Python model
tests/ple_ref.py and the fixtures tests/golden/ple/*.npz.  The GPU tests in tests/test_gpu_ple_exact.py rely on the oracle at
sizes the model cannot reach, so the two are pinned to each other here on every small shape.  No device is needed."""
import glob
import os
import random

import numpy as np
import pytest

import gf2util as g
import ple_ref as R
from ple_cases import low_rank, structured

HERE = os.path.dirname(os.path.abspath(__file__))


def model(a, m, n, pluq):
    rank, P, Q, out = R.ple(R.rows_of(a, n), n, pluq)
    return rank, P, Q, R.words_of_rows(out, n)


def same(got, want):
    assert got[0] == want[0], ("rank", got[0], want[0])
    assert list(got[1]) == list(want[1]), "P differs"
    assert list(got[2]) == list(want[2]), "Q differs"
    assert np.array_equal(got[3], want[3]), "in-place result differs"


@pytest.mark.parametrize("m", range(1, 71))
def test_every_shape_to_70(m):
    for n in range(1, 71):
        a = g.random_words(m, n, 1000 * m + n)
        if (m + n) % 3 == 0:  # rank-deficient on a third of the shapes
            a = low_rank(m, n, min(m, n) // 2, m + n)
        for pluq in (False, True):
            same(g.o_ple(a, m, n, pluq), model(a, m, n, pluq))


@pytest.mark.parametrize("m,n", [(64, 64), (65, 129), (129, 65), (200, 300), (300, 200), (300, 300)])
@pytest.mark.parametrize("pluq", [False, True])
def test_random_and_low_rank_to_300(m, n, pluq):
    for r in (None, 0, 1, 63, 64, 65, 130):
        if r is not None and r > min(m, n):
            continue
        a = g.random_words(m, n, m * n) if r is None else low_rank(m, n, r, r + m)
        same(g.o_ple(a, m, n, pluq), model(a, m, n, pluq))


@pytest.mark.parametrize("m,n", [(1, 70), (63, 65), (150, 90), (90, 150)])
@pytest.mark.parametrize("pluq", [False, True])
def test_structured(m, n, pluq):
    for a in structured(m, n):
        same(g.o_ple(a, m, n, pluq), model(a, m, n, pluq))


def test_golden_fixtures():
    files = sorted(glob.glob(os.path.join(HERE, "golden", "ple", "*.npz")))
    assert files
    for f in files:
        z = np.load(f)
        m, n = int(z["m"]), int(z["n"])
        for pluq, key in ((False, "ple"), (True, "pluq")):
            same(g.o_ple(z["a"], m, n, pluq), (int(z["rank"]), z["P"].tolist(), z["Q"].tolist(), z[key]))


def test_ple_ignores_dirty_excess_bits():
    m, n = 50, 70
    a = g.random_words(m, n, 5)
    dirty = a.copy()
    dirty[:, -1] |= np.uint64(0xFFFF) << np.uint64(n % 64)
    rank, P, Q, out = g.o_ple(dirty, m, n, False)
    out[:, -1] &= np.uint64((1 << (n % 64)) - 1)
    same((rank, P, Q, out), model(a, m, n, False))


def rand_perm(size, length, rng):
    return [rng.randrange(i, size) for i in range(length)]


@pytest.mark.parametrize("m,n", [(1, 1), (5, 9), (64, 64), (70, 130), (130, 70), (200, 257)])
def test_apply_p_against_model(m, n):
    rng = random.Random(m * 1000 + n)
    a = g.random_words(m, n, m + n)
    rows = R.rows_of(a, n)
    for right in (False, True):
        size = n if right else m
        for length in (size, max(size - 3, 0), size + 5):  # full, shorter (len < rows) and longer than the matrix
            perm = rand_perm(size, min(length, size), rng) + [0] * max(length - size, 0)
            for trans in (False, True):
                want = R.apply_right(rows, perm, n, trans) if right else R.apply_left(rows, perm, trans)
                got = g.o_apply_p(a, m, n, perm, right=right, trans=trans)
                assert np.array_equal(got, R.words_of_rows(want, n)), (right, trans, length)


def test_ple_p_and_q_reproduce_the_factors():
    """apply_p(A0, P) = L E; and with Q, right_trans: = L U (M4RI's test identity) -- on the oracle's own output"""
    m, n = 120, 190
    a = low_rank(m, n, 70, 3)
    for pluq in (False, True):
        rank, P, Q, out = g.o_ple(a, m, n, pluq)
        L, U = R.split_le(R.rows_of(out, n), rank, n)
        lhs = g.o_apply_p(a, m, n, P)
        if pluq:
            lhs = g.o_apply_p(lhs, m, n, Q, right=True, trans=True)
        assert R.rows_of(lhs, n) == R.mul(L, U)
