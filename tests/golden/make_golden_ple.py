"""Writes tests/golden/ple/*.npz: inputs of mzd_ple / mzd_pluq with the expected rank, P, Q and in-place results, computed by
the pure-Python model tests/ple_ref.py.  Run from the repository root: python tests/golden/make_golden_ple.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ple_ref as R  # noqa: E402


def rand_rows(m, n, rng):
    return [int.from_bytes(rng.bytes((n + 7) // 8), "little") & ((1 << n) - 1) for _ in range(m)]


def low_rank_rows(m, n, r, rng):
    X, Y = rand_rows(m, r, rng), rand_rows(r, n, rng)
    return R.mul(X, Y)


def main():
    out = os.path.join(HERE, "ple")
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(20261016)
    cases = [("random_63x65", rand_rows(63, 65, rng), 65),
             ("random_65x129", rand_rows(65, 129, rng), 129),
             ("rank40_200x150", low_rank_rows(200, 150, 40, rng), 150),
             ("rank64_130x260", low_rank_rows(130, 260, 64, rng), 260)]
    for name, rows, n in cases:
        m = len(rows)
        rank, P, Q, ple = R.ple(rows, n)
        _, _, _, pluq = R.ple(rows, n, pluq=True)
        np.savez_compressed(os.path.join(out, name + ".npz"), m=m, n=n, a=R.words_of_rows(rows, n), rank=rank,
                            P=np.array(P, dtype=np.int32), Q=np.array(Q, dtype=np.int32), ple=R.words_of_rows(ple, n),
                            pluq=R.words_of_rows(pluq, n))


if __name__ == "__main__":
    main()
