"""The four-level Strassen plan folds its 2401 leaf products into C in ONE launch (gf2_strassen_merge4_kernel): a workgroup of seven
waves takes 64 consecutive word positions of the leaves, wave q0 walks top-level group q0, and the 256 results of a position are
sums in LDS that every wave adds into.  With four levels m % 16 == 0 and l, n % 2048 == 0; h = m / 16 leaf rows, w = n / 1024 leaf
words, positions = h * w, blocks of 64.  The shapes are the smallest that reach each place where the kernel can go wrong (CASES).
Every product is compared bit for bit with plain Four Russians, which is held to the oracle on sampled rows; the accumulate form
and a second run into the same scratch likewise, and the launch census says that the new kernel ran and the single-level merge,
which the plan used to end with, did not."""
import numpy as np
import pytest

import gf2util as g
from census_util import assert_route, census

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from m4ri_rust_amd import device
    device.require_gpu()
    return device


@pytest.fixture(scope="module")
def lib():
    import m4ri_rust_amd as pkg
    return pkg._lib.lib()


def launched(before, after, name):
    return sum(v - before.get(k, 0) for k, v in after.items() if name in k)


CASES = [
    (16, 2048, 2048),       # 2 positions: one partial block, 62 idle lanes at every barrier and at the write-out
    (1040, 2048, 4096),     # 260: four full blocks and a tail of 4
    (1024, 2048, 6144),     # 384: full blocks whose boundaries fall inside a row (w = 6)
    (32768, 2048, 32768),   # 65536: 1024 blocks, more than the grid -- several blocks per workgroup (sums cleared in between)
]


@pytest.mark.parametrize("m,l,n", CASES)
def test_four_levels_match_m4rm_and_oracle(dev, lib, m, l, n):
    A, B = dev.DMat.random(m, l, 41), dev.DMat.random(l, n, 42)
    ref = dev.mul(A, B, algo="m4rm")
    rows = sorted({r for r in (0, 1, 63, 64, m // 2, m - 1) if r < m})  # (m = 16 has no rows 63 and 64)
    a_rows = np.ascontiguousarray(g.random_words(m, l, 41)[rows])
    assert np.array_equal(ref.to_words()[rows], g.o_mul_m4rm(a_rows, g.random_words(l, n, 42), len(rows), l, n))
    k0 = census(lib)
    C1 = dev.mul(A, B, algo="strassen", param=4)
    k1 = census(lib)
    assert dev.equal(C1, ref), "product"
    assert_route(k0, k1, ["gf2_strassen_merge4_kernel"])
    C2 = dev.DMat.random(m, n, 43)
    expect = dev.add(C2, ref)
    dev.mul(A, B, C=C2, accumulate=True, algo="strassen", param=4)
    assert dev.equal(C2, expect), "accumulate"
    # a second run into the same scratch gives the same bits (no dependence on what the arena held)
    assert dev.equal(dev.mul(A, B, algo="strassen", param=4), ref), "repeat"


def test_accumulate_into_a_column_window(dev, lib):
    """C is a column window of a wider matrix (row stride larger than its width), starting at a multiple of 128 columns so that
    the four-level route is kept.  Every word of the parent is compared: the window, and the columns outside it unchanged."""
    m, l, n, c0, extra = 1040, 2048, 4096, 128, 256
    A, B = dev.DMat.random(m, l, 51), dev.DMat.random(l, n, 52)
    ref = dev.mul(A, B, algo="m4rm")
    parent = dev.DMat.random(m, n + extra, 53)
    expect = parent.clone()
    dev.copy_block(expect, 0, c0, ref, 0, 0, m, n, accumulate=True)
    view = dev.DMat.wrap(parent.s.data + 8 * (c0 // 64), m, n, parent.ld, keep=parent)
    assert view.ld > n // 64
    k0 = census(lib)
    dev.mul(A, B, C=view, accumulate=True, algo="strassen", param=4)
    assert_route(k0, census(lib), ["gf2_strassen_merge4_kernel"])
    assert dev.equal(parent, expect), "window or the columns beside it"
    # and the overwriting form into the same window
    dev.copy_block(expect, 0, c0, ref, 0, 0, m, n)
    dev.mul(A, B, C=view, algo="strassen", param=4)
    assert dev.equal(parent, expect), "overwrite: window or the columns beside it"


def test_four_levels_launch_merge4_and_no_single_level_merge(dev, lib):
    m, l, n = 1040, 2048, 4096
    A, B = dev.DMat.random(m, l, 61), dev.DMat.random(l, n, 62)
    k0 = census(lib)
    dev.mul(A, B, algo="strassen", param=4)
    k1 = census(lib)
    assert launched(k0, k1, "gf2_strassen_merge4_kernel") == 1
    assert launched(k0, k1, "gf2_strassen_merge_kernel") == 0, "the level-1 products were written and merged"
    assert launched(k0, k1, "gf2_strassen_merge3_kernel") == 0
