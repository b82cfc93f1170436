"""The fused Strassen passes with a virtual fourth level walk their workgroups group-fastest: the seven workgroups that read one
position block of the grandparent quadrants run side by side (gf2_strassen_split3_kernel).  These shapes give both sides every
kind of grid -- one position block, counts that are no multiple of seven or eight, the 16 x 16 tiled A path and the lane-per-row
packed one -- and a padded shape; the single-level and three-level merges store with non-temporal stores into the caller's C,
accumulate form included.  Every product has the bits of plain Four Russians and, on sampled rows, of the oracle."""
import numpy as np
import pytest

import gf2util as g

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from m4ri_rust_amd import device
    device.require_gpu()
    return device


# (m, l, n, levels): position blocks of the A / B split at 4 levels in the comments (h * w / 256, h = rows / 16, w = words / 16)
CASES = [
    (1024, 4096, 4096, 4),     # A 1 block, B 4
    (3072, 6144, 2048, 4),     # A 5 (packed, not tiled), B 3
    (5120, 2048, 10240, 4),    # A 3, B 5
    (16384, 32768, 16384, 4),  # A 128 (tiled), B 128
    (6000, 10000, 7000, 4),    # does not divide: padded or peeled plan
    (4096, 8192, 6144, 1),     # single-level merge into C
    (8192, 4096, 8192, 3),     # three-level merge into C
]


@pytest.mark.parametrize("m,l,n,levels", CASES)
def test_strassen_passes_match_m4rm_and_oracle(dev, m, l, n, levels):
    A, B = dev.DMat.random(m, l, 31), dev.DMat.random(l, n, 32)
    ref = dev.mul(A, B, algo="m4rm")
    rows = [0, 1, 63, 64, m // 2, m - 1]
    a_rows = np.ascontiguousarray(g.random_words(m, l, 31)[rows])
    assert np.array_equal(ref.to_words()[rows], g.o_mul_m4rm(a_rows, g.random_words(l, n, 32), len(rows), l, n))
    C1 = dev.mul(A, B, algo="strassen", param=levels)
    assert dev.equal(C1, ref), "product"
    C2 = dev.DMat.random(m, n, 33)
    expect = dev.add(C2, ref)
    dev.mul(A, B, C=C2, accumulate=True, algo="strassen", param=levels)
    assert dev.equal(C2, expect), "accumulate"
    # a second run into the same scratch gives the same bits (no dependence on what the arena held)
    assert dev.equal(dev.mul(A, B, algo="strassen", param=levels), ref), "repeat"
