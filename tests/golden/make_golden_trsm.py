"""Writes tests/golden/trsm/*.npz: a random n x n matrix t (its strict lower triangle is L, its strict upper triangle is U, the
diagonal counts as 1), right-hand sides b_left (n x k) and b_right (k x n), and the four solutions, computed by the numpy
substitution of tests/trsm_ref.py.  Run from the repository root: python tests/golden/make_golden_trsm.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import gf2util as g  # noqa: E402
import trsm_ref as R  # noqa: E402


def main():
    out = os.path.join(HERE, "trsm")
    os.makedirs(out, exist_ok=True)
    k = 70
    for n in (63, 65, 200):
        tb = R.random_bits(n, n, 20261017 + n)
        bl, br = g.random_words(n, k, 7 * n), g.random_words(k, n, 7 * n + 1)
        sol = {}
        for upper, right in R.VARIANTS:
            rows, cols = R.b_shape(n, k, right)
            x = R.solve(tb, br if right else bl, rows, cols, upper, right)
            R.check_product(tb, x, br if right else bl, rows, cols, upper, right)
            sol["x_" + R.name(upper, right)] = x
        np.savez_compressed(os.path.join(out, "random_%dx%d.npz" % (n, k)), n=n, k=k, t=g.bits_to_words(tb), b_left=bl,
                            b_right=br, **sol)


if __name__ == "__main__":
    main()
