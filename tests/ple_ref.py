"""Pure-Python PLE / PLUQ of the contract in INTEGRATION.md section 3 (rows as Python ints, bit j = column j): column-greedy
elimination, the pivot of column c being the first remaining row, in input order, with bit c.  Shares no code with the
oracle or the library; used by tests/test_ple_host.py, tests/test_gpu_ple.py and tests/golden/make_golden_ple.py."""
import numpy as np


def rows_of(words, ncols):
    """(m, w) uint64 array -> list of ints (excess bits dropped)."""
    mask = (1 << ncols) - 1
    out = []
    for r in np.asarray(words, dtype=np.uint64):
        v = 0
        for j, x in enumerate(r.tolist()):
            v |= int(x) << (64 * j)
        out.append(v & mask)
    return out


def words_of_rows(rows, ncols):
    w = max((ncols + 63) // 64, 1)
    a = np.zeros((len(rows), w), dtype=np.uint64)
    for i, v in enumerate(rows):
        for j in range(w):
            a[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return a


def transpositions(sigma):
    """sigma[i] = input row at position i -> P with apply_p_left(A0, P) == A0[sigma]."""
    m = len(sigma)
    pos, at, P = list(range(m)), list(range(m)), [0] * m
    for i in range(m):
        p = pos[sigma[i]]
        P[i] = p
        a, b = at[i], at[p]
        at[i], at[p] = at[p], at[i]
        pos[a], pos[b] = p, i
    return P


def apply_left(rows, P, trans=False):
    rows = list(rows)
    n = min(len(P), len(rows))
    for i in (reversed(range(n)) if trans else range(n)):
        rows[i], rows[P[i]] = rows[P[i]], rows[i]
    return rows


def swap_bits(v, a, b):
    if ((v >> a) ^ (v >> b)) & 1:
        v ^= (1 << a) | (1 << b)
    return v


def apply_right(rows, P, ncols, trans=False):
    """Column swaps (i, P[i]): descending for right, ascending for right_trans."""
    n = min(len(P), ncols)
    order = range(n) if trans else reversed(range(n))
    order = list(order)
    out = []
    for v in rows:
        for i in order:
            v = swap_bits(v, i, P[i])
        out.append(v)
    return out


def ple(rows, ncols, pluq=False):
    """-> (rank, P, Q, out rows): out is the in-place result of mzd_ple (or mzd_pluq)."""
    m = len(rows)
    cur = list(rows)
    L = [0] * m
    rest = list(range(m))
    order, q = [], []
    for c in range(ncols):
        p = next((r for r in rest if (cur[r] >> c) & 1), None)
        if p is None:
            continue
        k = len(order)
        rest.remove(p)
        order.append(p)
        q.append(c)
        e = cur[p]
        for r in rest:
            if (cur[r] >> c) & 1:
                cur[r] ^= e
                L[r] |= 1 << k
    rank = len(order)
    sigma = order + rest
    out = []
    for i, src in enumerate(sigma):
        if i < rank:
            e = cur[src]
            if pluq:
                for t in range(rank):
                    e = swap_bits(e, t, q[t])
            out.append((L[src] & ((1 << i) - 1)) | e)
        else:
            out.append(L[src] & ((1 << rank) - 1))
    Q = q + list(range(rank, ncols))
    return rank, transpositions(sigma), Q, out


def split_le(out, rank, ncols):
    """In-place result -> (L rows: m x rank, E/U rows: rank x ncols)."""
    L = [(v & ((1 << min(i, rank)) - 1)) | ((1 << i) if i < rank else 0) for i, v in enumerate(out)]
    U = [out[i] & ~((1 << i) - 1) & ((1 << ncols) - 1) for i in range(rank)]
    return L, U


def mul(L, U):
    """(rows of L over len(U) columns) x (rows of U) over GF(2)."""
    res = []
    for v in L:
        acc, k = 0, 0
        while v:
            if v & 1:
                acc ^= U[k]
            v >>= 1
            k += 1
        res.append(acc)
    return res


def solve_free_zero(rows, ncols, brows):
    """Unique X with A0 X = B over the row-rank-profile subsystem and free variables 0 (consistent systems)."""
    rank, P, Q, out = ple(rows, ncols, pluq=True)
    b = apply_left(brows, P)
    for i in range(rank):
        for k in range(i):
            if (out[i] >> k) & 1:
                b[i] ^= b[k]
    ok = True
    for i in range(rank, len(rows)):
        v = b[i]
        for k in range(rank):
            if (out[i] >> k) & 1:
                v ^= b[k]
        ok = ok and v == 0
    for i in reversed(range(rank)):
        for k in range(i + 1, rank):
            if (out[i] >> k) & 1:
                b[i] ^= b[k]
    z = b[:rank] + [0] * (ncols - rank)
    return apply_left(z, Q, trans=True), ok
