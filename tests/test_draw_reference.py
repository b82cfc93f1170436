"""The yardstick of the draw tests (tests/draw_ref.py) against what include/m4ri_hip_draw.h says, on the CPU: the published known
answers of Philox4x32-10, the bit-sliced comparison against the per-bit definition, the subset rule (distinct, in range, uniform over
the ordered pairs at k = 2, n = 4, -1 behind a short max_rounds), the indices and the permutation's ties."""
import itertools

import numpy as np
import pytest

import draw_ref as dr

THRS = [0, 1, 0x20000000, 0x80000000, 0x12345679, 0xFFFFFFFF]

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def philox_scalar(ctr, key):
    """the textbook form on Python integers, independent of the array code"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("ctr,key,out", KNOWN)
def test_known_answers(ctr, key, out):
    want = [int(x, 16) for x in out.split()]
    assert philox_scalar(ctr, key) == want
    assert [int(x[0]) for x in dr.philox(*ctr, *key)] == want


def test_arrays_of_counters_equal_the_scalar_form():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, (4, 50), dtype=np.uint64)
    got = np.array(dr.philox(c[0], c[1], c[2], c[3], 0x12345678, 0x9ABCDEF0))
    for j in range(50):
        assert list(got[:, j]) == philox_scalar([int(v) for v in c[:, j]], (0x12345678, 0x9ABCDEF0))
    seed, at = 0xDEADBEEFCAFEF00D, (1 << 63) + 12345
    assert [int(x[0]) for x in dr.block(seed, [at], 7, 3)] == philox_scalar([at & 0xFFFFFFFF, at >> 32, 7, 3], (seed & 0xFFFFFFFF, seed >> 32))


def test_mulhi64():
    rng = np.random.default_rng(2)
    lo, hi = rng.integers(0, 1 << 32, (2, 200), dtype=np.uint64)
    lo[:4], hi[:4] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF], [0, 0, 0xFFFFFFFF, 0xFFFFFFFF]
    for n in (1, 2, 3, 1000, (1 << 31) - 1, (1 << 32) - 1):
        slow = dr.below(lo, hi, n)
        assert np.array_equal(dr.below_fast(lo, hi, n).astype(np.int64), slow) and slow.min() >= 0 and slow.max() < n
        assert slow[3] == n - 1 and slow[0] == 0      # X = 2^64 - 1 gives n - 1, X = 0 gives 0


@pytest.mark.parametrize("thr", THRS)
def test_the_bit_sliced_recurrence_is_the_comparison(thr):
    widx = np.array([0, 1, 5, (1 << 32) - 1, 1 << 32, (1 << 40) + 3], dtype=np.uint64)
    got, calls = dr.bernoulli_words(77, widx, thr)
    assert np.array_equal(got, dr.bernoulli_words_by_bits(77, widx, thr))
    assert calls == {0: 0, 1: 16, 0x20000000: 2, 0x80000000: 1, 0x12345679: 16, 0xFFFFFFFF: 16}[thr]
    if thr == 0:
        assert not got.any()
    if thr == 0xFFFFFFFF:
        assert all(bin(int(x)).count("1") == 64 for x in got)      # a zero bit has probability 2^-32


def test_bernoulli_density_and_positions():
    words = dr.bernoulli(5, 0x20000000, 200, 640)           # tau = 1/8 over 128000 bits: sigma = 118
    ones = sum(bin(int(x)).count("1") for x in words.reshape(-1))
    assert abs(ones - 16000) < 600
    # a block of the whole, and a matrix with excess bits
    assert np.array_equal(dr.bernoulli(5, 0x20000000, 7, 128, row0=11, col_word0=3, full_ncols=640), words[11:18, 3:5])
    part = dr.bernoulli(5, 0x20000000, 7, 100, row0=11, col_word0=3, full_ncols=640)
    assert np.array_equal(part[:, 0], words[11:18, 3]) and np.array_equal(part[:, 1], words[11:18, 4] & np.uint64((1 << 36) - 1))
    # the word index wraps into counter word 1
    far = dr.bernoulli(5, 1, 3, 64 * 1024, row0=(1 << 22) - 1, full_ncols=64 * 1024)
    assert np.array_equal(far[1, :2], dr.bernoulli_words(5, [1 << 32, (1 << 32) + 1], 1)[0])


def test_indices():
    for n in (1, 2, 3, 1000, (1 << 31) - 1):
        a = dr.indices(3, 1001, n)
        assert a.dtype == np.int32 and len(a) == 1001 and a.min() >= 0 and a.max() < n
        assert np.array_equal(dr.indices(3, 64, n), a[:64]) and np.array_equal(dr.indices(3, 63, n), a[:63])
    assert len(dr.indices(3, 0, 5)) == 0
    counts = np.bincount(dr.indices(4, 30000, 3), minlength=3)
    assert counts.min() > 9600 and counts.max() < 10400        # sigma = 82
    x = dr.block(3, [2], 0, dr.TAG_INDICES)
    assert list(dr.indices(3, 6, 1000)[4:6]) == [int(dr.below(x[0], x[1], 1000)[0]), int(dr.below(x[2], x[3], 1000)[0])]


@pytest.mark.parametrize("k,n,batch", [(1, 2, 50), (2, 4, 200), (8, 16, 200), (64, 128, 20), (65, 130, 5), (64, 1 << 20, 20)])
def test_subsets_are_distinct(k, n, batch):
    sub, unfinished = dr.subsets(21, batch, k, n)
    assert unfinished == 0 and sub.shape == (batch, k) and sub.min() >= 0 and sub.max() < n
    assert all(len(set(row)) == k for row in sub)


def test_subsets_are_uniform_over_the_ordered_pairs():
    sub, unfinished = dr.subsets(9, 6000, 2, 4)
    assert unfinished == 0
    counts = {p: 0 for p in itertools.permutations(range(4), 2)}
    for a, b in sub:
        counts[(int(a), int(b))] += 1
    assert len(counts) == 12 and 400 <= min(counts.values()) and max(counts.values()) <= 600, counts     # 500 each, sigma = 21


def test_subsets_follow_the_sequential_rule():
    """round by round on one subset, written out once more: the candidates, what is taken, who is rejected"""
    seed, k, n = 5, 8, 16
    sub, _ = dr.subsets(seed, 40, k, n)
    for g in range(40):
        value, rounds = {}, 0
        while len(value) < k:
            cand = {t: int(dr.subset_candidates(seed, [g * k + t], rounds, n)[0]) for t in range(k) if t not in value}
            taken, seen = set(value.values()), set()
            for t in sorted(cand):
                if cand[t] not in taken and cand[t] not in seen:
                    value[t] = cand[t]
                seen.add(cand[t])
            rounds += 1
        assert [value[t] for t in range(k)] == list(sub[g])
    one, unfinished = dr.subsets(seed, 40, k, n, max_rounds=1)
    assert 0 < unfinished <= 40 and unfinished == int((one < 0).any(axis=1).sum())
    assert np.array_equal(one[one >= 0], sub[one >= 0])              # what settled in round 0 stays
    assert all(len(set(r[r >= 0])) == (r >= 0).sum() for r in one)


def test_permutation():
    for n in (0, 1, 2, 255, 256, 257):
        p = dr.permutation(1, n)
        assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(n))
    for seed in (1, 2, 3):
        keys = dr.perm_keys(seed, 70000)
        p = dr.permutation(seed, 70000)
        assert keys.min() >= 0 and keys.max() < 1 << 30
        sk = keys[p]
        ties = np.flatnonzero(np.diff(sk) == 0)
        assert len(ties) >= 1                                     # 70000^2 / 2^31 = 2.3 expected
        assert np.all(np.diff(sk) >= 0) and np.all(np.diff(p)[ties] > 0)     # ties in index order
        assert np.array_equal(np.sort(p), np.arange(70000))
