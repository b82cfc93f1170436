"""The reference of the GPU tests of the Walsh-Hadamard transform (tests/wht_ref.py) against the definition, without the library: the
butterfly loop equals the matrix (-1)^popcount(s & v) applied in exact integers and reduced modulo 2^32, for every k <= 10."""
import numpy as np
import pytest

import wht_ref as wr


def by_definition(f, k):
    H = wr.definition_matrix(k)
    exact = [int(sum(int(h) * int(x) for h, x in zip(row, f))) for row in H] if k <= 6 else None
    # int64 wraps modulo 2^64, of which 2^32 is a divisor: the product below is exact modulo 2^32
    fast = (H @ f.astype(np.int64)) & wr.MASK
    if exact is not None:
        assert [e % (1 << 32) for e in exact] == [int(x) for x in fast]
    return fast


@pytest.mark.parametrize("k", range(11))
def test_butterfly_loop_equals_the_definition(k):
    rng = np.random.default_rng(100 + k)
    n = 1 << k
    inputs = [rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64), np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64),
              rng.integers(-3, 4, n, dtype=np.int64)]
    for f in inputs:
        got = wr.wht_reference(f, k)
        assert got.dtype == np.int64 and got.shape == (n,) and got.min() >= 0 and got.max() <= wr.MASK
        assert np.array_equal(got, by_definition(f, k))


@pytest.mark.parametrize("k", [0, 1, 4, 10])
def test_closed_forms(k):
    n = 1 << k
    s = np.arange(n, dtype=np.int64)
    assert np.array_equal(wr.wht_reference(np.ones(n, dtype=np.int64), k), np.where(s == 0, n, 0))
    rng = np.random.default_rng(k)
    for sign in (1, -1):
        v = int(rng.integers(0, n))
        f = np.zeros(n, dtype=np.int64)
        f[v] = sign
        want = wr.delta_transform(s, v, sign, k)
        assert set(np.unique(want)) <= {-1, 1}
        assert np.array_equal(wr.wht_reference(f, k), want & wr.MASK)
    # twice the transform is f << k
    f = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64)
    assert np.array_equal(wr.wht_reference(wr.wht_reference(f, k), k), (f << k) & wr.MASK)
    assert np.array_equal(wr.as_int32(np.array([0, 1, (1 << 31), wr.MASK])), np.array([0, 1, -(1 << 31), -1], dtype=np.int32))


def test_the_loop_runs_on_torch_tensors_too():
    import torch
    rng = np.random.default_rng(7)
    for k in (0, 3, 9):
        f = rng.integers(-(1 << 31), 1 << 31, 1 << k, dtype=np.int64)
        assert np.array_equal(wr.wht_reference(torch.from_numpy(f), k).numpy(), wr.wht_reference(f, k))
        s = np.arange(1 << k, dtype=np.int64)
        assert np.array_equal(wr.delta_transform(torch.from_numpy(s), 5 % (1 << k), -1, k).numpy(), wr.delta_transform(s, 5 % (1 << k), -1, k))
