"""The yardstick of tests/test_gpu_wht.py, checked on its own by tests/test_wht_reference.py: the Walsh-Hadamard transform as a plain
butterfly loop in int64, reduced modulo 2^32, and the closed forms the GPU tests use.  Nothing here calls the library.

wht_reference() only reshapes, adds, subtracts and concatenates, so it runs unchanged on a numpy array and on a torch tensor: the
GPU tests hand it a device tensor where a numpy run of 2^27 or 2^28 int64 would take most of a minute."""
import numpy as np

MASK = (1 << 32) - 1


def wht_reference(f, k):
    """F[s] = sum over v of (-1)^popcount(s & v) f[v] for 2^k int64 values f, reduced to [0, 2^32) after every level (so nothing
    overflows: |a +- b| < 2^33); f is a numpy array or a torch tensor of int64"""
    lib = np if isinstance(f, np.ndarray) else __import__("torch")
    f = f & MASK
    for level in range(k):
        h = 1 << level
        pairs = f.reshape(-1, 2, h)
        a, b = pairs[:, 0, :], pairs[:, 1, :]
        f = lib.stack([a + b, a - b], 1).reshape(-1) & MASK
    return f


def as_int32(f):
    """values in [0, 2^32) as the int32 with the same bits (numpy)"""
    return np.asarray(f, dtype=np.int64).astype(np.uint32).view(np.int32)


def definition_matrix(k):
    """H[s][v] = (-1)^popcount(s & v), 2^k x 2^k int64"""
    i = np.arange(1 << k, dtype=np.int64)
    x = i[:, None] & i[None, :]
    par = np.zeros_like(x)
    for b in range(k):
        par ^= (x >> b) & 1
    return 1 - 2 * par


def parity(x, k):
    """popcount(x) mod 2 for 0 <= x < 2^k, k <= 32, by folding halves; numpy array or torch tensor of int64"""
    assert k <= 32
    for shift in (16, 8, 4, 2, 1):
        x = x ^ (x >> shift)
    return x & 1


def delta_transform(s, v, sign, k):
    """the transform of sign * (unit vector at v), at the indices s: sign * (-1)^<s, v>"""
    return sign * (1 - 2 * parity(s & v, k))
