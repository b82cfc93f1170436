"""The yardstick of the draw tests (include/m4ri_hip_draw.h): Philox4x32-10 and the four contracts built on it, in numpy and plain
Python, written from the text of the header and not from the kernels.  Arrays of counters go through the rounds at once; the subset
rule is the sequential one, position by position.  tests/test_draw_reference.py checks it against the published known answers and
against the per-bit definitions."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG_BERNOULLI, TAG_INDICES, TAG_SUBSETS, TAG_PERMUTATION = 1, 2, 3, 4
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64 -> (x0, x1, x2, x3) as uint64 arrays below 2^32"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK32 for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c0           # below 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def block(seed, at, c2, tag):
    """the block of the 64-bit positions `at` under a seed: key (seed low, seed high), counter (at low, at high, c2, tag)"""
    at = np.atleast_1d(np.asarray(at, dtype=np.uint64))
    return philox(at & MASK32, at >> S32, c2, tag, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def below(lo, hi, n):
    """mulhi64(lo | hi << 32, n) for arrays of 32-bit halves: Python integers, so the 128-bit product is exact"""
    return np.array([(((int(h) << 32) | int(l)) * int(n)) >> 64 for l, h in zip(np.atleast_1d(lo), np.atleast_1d(hi))], dtype=np.int64)


def below_fast(lo, hi, n):
    """the same in numpy for n < 2^32 (test_draw_reference.py holds it to below())"""
    n = np.uint64(n)
    return (((lo * n) >> S32) + hi * n) >> S32


# ---- Bernoulli

def planes(seed, widx):
    """R[m], m < 32, of the words widx: (32, len(widx)) uint64"""
    R = []
    for q in range(16):
        x0, x1, x2, x3 = block(seed, widx, q, TAG_BERNOULLI)
        R += [x0 | (x1 << S32), x2 | (x3 << S32)]
    return np.array(R)


def bernoulli_words_by_bits(seed, widx, thr):
    """the definition: bit i of the word is U_i < thr, U_i = the number whose bit m is bit i of R[m]"""
    R = planes(seed, widx)
    out = np.zeros(R.shape[1], dtype=np.uint64)
    for i in range(64):
        U = np.zeros(R.shape[1], dtype=np.uint64)
        for m in range(32):
            U |= ((R[m] >> np.uint64(i)) & np.uint64(1)) << np.uint64(m)
        out |= (U < np.uint64(thr)).astype(np.uint64) << np.uint64(i)
    return out


def bernoulli_words(seed, widx, thr):
    """the same through the bit-sliced recurrence, least significant plane first, with the calls below the lowest set bit of thr
    skipped -> (words, Philox calls made per word)"""
    widx = np.atleast_1d(np.asarray(widx, dtype=np.uint64))
    lt = np.zeros(len(widx), dtype=np.uint64)
    if thr == 0:
        return lt, 0
    q0 = ((thr & -thr).bit_length() - 1) // 2
    for q in range(q0, 16):
        x0, x1, x2, x3 = block(seed, widx, q, TAG_BERNOULLI)
        for m, R in ((2 * q, x0 | (x1 << S32)), (2 * q + 1, x2 | (x3 << S32))):
            lt = (~R | lt) if (thr >> m) & 1 else (~R & lt)
    return lt, 16 - q0


def bernoulli(seed, thr, nrows, ncols, row0=0, col_word0=0, full_ncols=0):
    """the noise of an nrows x ncols matrix (or block) as packed words, excess bits zero"""
    w = (ncols + 63) // 64
    fullw = (full_ncols + 63) // 64 if full_ncols else w
    widx = ((row0 + np.arange(nrows, dtype=object))[:, None] * fullw + col_word0 + np.arange(w, dtype=object)[None, :])
    widx = np.array(widx.reshape(-1) % (1 << 64), dtype=np.uint64)
    words = bernoulli_words(seed, widx, thr)[0].reshape(nrows, w)
    if ncols % 64 and nrows:
        words[:, -1] &= np.uint64((1 << (ncols % 64)) - 1)
    return words


# ---- indices

def indices(seed, count, n):
    p = np.arange((count + 1) // 2, dtype=np.uint64)
    x0, x1, x2, x3 = block(seed, p, 0, TAG_INDICES)
    out = np.empty(2 * len(p), dtype=np.int64)
    out[0::2] = below_fast(x0, x1, n)
    out[1::2] = below_fast(x2, x3, n)
    return out[:count].astype(np.int32)


# ---- subsets

def subset_candidates(seed, at, a, n):
    x0, x1, _, _ = block(seed, at, a, TAG_SUBSETS)
    return below_fast(x0, x1, n).astype(np.int64)


def subsets(seed, batch, k, n, max_rounds=0):
    """-> (sub as (batch, k) int32 with -1 where a position has not settled, the number of subsets with such a position).  The rule
    of the header, one subset at a time: in round a the open positions draw, and are visited in ascending order"""
    rounds = max_rounds or 64
    sub = np.full((batch, k), -1, dtype=np.int64)
    open_ = np.ones((batch, k), dtype=bool)
    at = np.arange(batch * k, dtype=np.uint64).reshape(batch, k)
    for a in range(rounds):
        gs = np.flatnonzero(open_.any(axis=1))
        if len(gs) == 0:
            break
        cand = np.full((batch, k), -1, dtype=np.int64)
        cand[open_] = subset_candidates(seed, at[open_], a, n)
        for g in gs:
            taken = set(int(v) for v in sub[g][~open_[g]])     # settled in an earlier round
            seen = set()                                       # drawn in this round by an open position below
            for t in np.flatnonzero(open_[g]):
                v = int(cand[g, t])
                if v not in taken and v not in seen:
                    sub[g, t] = v
                seen.add(v)
            open_[g] = sub[g] < 0
    return sub.astype(np.int32), int(open_.any(axis=1).sum())


# ---- permutation

def perm_keys(seed, n):
    return (block(seed, np.arange(n, dtype=np.uint64), 0, TAG_PERMUTATION)[0] & np.uint64((1 << 30) - 1)).astype(np.int64)


def permutation(seed, n):
    return np.argsort(perm_keys(seed, n), kind="stable").astype(np.int32)
