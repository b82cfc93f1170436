"""GPU tests of the batched elimination of small matrices (gf2_elim_batch.hip; gf2_echelonize_batch_dev, gf2_inverse_batch_dev
through device.echelonize_batch / inverse_batch).  Every stack is compared matrix by matrix with the CPU oracle (gf2util.o_echelonize,
o_inverse).  For full = 1 everything is unique, so the comparisons are bit-exact: the words, the ranks and the whole array of pivot
columns with its -1 entries.  The stacks live in torch tensors (row stride: the width rounded up to even), ranks / pivot columns /
singular flags in torch int32 tensors that hold a poison value before the call."""
import functools

import numpy as np
import pytest

import gf2util as g
from elim_batch_cases import INVERSE_SIZES, SHAPES
from stream_util import POISON, padded, run_pending

pytestmark = pytest.mark.gpu

INT_POISON = -77


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


@pytest.fixture(scope="module")
def dev(pkg):
    from m4ri_rust_amd import device
    return device


def to_gpu(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def ints(count):
    import torch
    return torch.full((max(count, 1),), INT_POISON, dtype=torch.int32, device="cuda")


def limit_of(ncols, ncols_limit):
    return ncols_limit if 0 < ncols_limit < ncols else ncols


def reference(words, m, ncols, full=True, ncols_limit=0):
    """the oracle, matrix by matrix -> (words, ranks, pivot columns padded with -1 to P = min(m, limit))"""
    batch = words.shape[0] // m
    P = min(m, limit_of(ncols, ncols_limit))
    out, ranks, piv = np.empty_like(words), np.zeros(batch, dtype=np.int32), np.full((batch, P), -1, dtype=np.int32)
    for b in range(batch):
        out[b * m:(b + 1) * m], ranks[b], cols = g.o_echelonize(words[b * m:(b + 1) * m], m, ncols, full=full, limit=ncols_limit)
        piv[b, :ranks[b]] = cols
    return out, ranks, piv


def run_batch(dev, words, m, ncols, full=True, ncols_limit=0):
    """the stack through the device call -> (words, ranks, pivot columns (batch, P)); the arrays are device arrays of the caller"""
    import torch
    batch = words.shape[0] // m
    P = min(m, limit_of(ncols, ncols_limit))
    t, tr, tp = to_gpu(padded(words)), ints(batch), ints(batch * P)
    dev.echelonize_batch(dev.DMat.from_torch(t, ncols), m, full=full, ncols_limit=ncols_limit, ranks=tr.data_ptr(), pivots=tp.data_ptr())
    torch.cuda.synchronize()
    got = to_host(t)
    assert not got[:, g.width(ncols):].any(), "the padding word of the even row stride was written"
    return got[:, :g.width(ncols)], tr.cpu().numpy()[:batch], tp.cpu().numpy()[:batch * P].reshape(batch, P)


def check_exact(dev, words, m, ncols, ncols_limit=0):
    got, ranks, piv = run_batch(dev, words, m, ncols, True, ncols_limit)
    ref, oranks, opiv = reference(words, m, ncols, True, ncols_limit)
    assert np.array_equal(ranks, oranks), (m, ncols, np.flatnonzero(ranks != oranks)[:8])
    assert np.array_equal(piv, opiv), (m, ncols)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, (m, ncols, "first differing matrix", bad[0] // m, "row", bad[0] % m)
    return oranks


# ---- random stacks: every shape of the case list ------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,ncols,batch", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_random_stacks(dev, m, ncols, batch):
    check_exact(dev, g.random_words(batch * m, ncols, 1000 + m + 7 * ncols), m, ncols)


def test_wrapper_allocates_and_returns_numpy(dev):
    """without arrays of the caller's the wrapper brings ranks and pivot columns back itself"""
    m, ncols, batch = 10, 10, 300
    words = g.random_words(batch * m, ncols, 5)
    A = dev.DMat.from_words(words, ncols)
    ranks, piv = dev.echelonize_batch(A, m)
    ref, oranks, opiv = reference(words, m, ncols)
    assert ranks.dtype == np.int32 and np.array_equal(ranks, oranks) and piv.shape == (batch, m) and np.array_equal(piv, opiv)
    assert np.array_equal(A.to_words()[:, :1], ref)
    Ainv, singular = dev.inverse_batch(dev.DMat.from_words(words, ncols), m)
    assert np.array_equal(singular, (oranks < m).astype(np.int32))
    inv0 = g.o_inverse(words[:m], m)
    b = int(np.flatnonzero(oranks == m)[0])
    assert np.array_equal(Ainv.to_words()[b * m:(b + 1) * m, :1], g.o_inverse(words[b * m:(b + 1) * m], m)) and (inv0 is None) == (oranks[0] < m)


# ---- mixed ranks in one batch ---------------------------------------------------------------------------------------------------------

def mixed_stack(m):
    """the special matrices, each followed by a random one"""
    w = g.width(m)
    eye = np.eye(m, dtype=np.uint8)
    half = g.words_to_bits(g.random_words((m + 1) // 2, m, 41), m)
    last = np.zeros((m, m), dtype=np.uint8)
    last[:, m - 1] = g.words_to_bits(g.random_words(m, 1, 42), 1)[:, 0] | (np.arange(m) == m - 1)
    special = [np.zeros((m, w), dtype=np.uint64), g.bits_to_words(eye), g.bits_to_words(eye[::-1].copy()),
               g.bits_to_words(np.ones((m, m), dtype=np.uint8)), g.bits_to_words(np.repeat(half, 2, axis=0)[:m].copy()), g.bits_to_words(last)]
    for r in (1, m // 2, m - 1):
        special.append(g.o_mul_naive(g.random_words(m, r, 50 + r), g.random_words(r, m, 60 + r), m, r, m))
    parts = []
    for i, s in enumerate(special):
        parts += [s, g.random_words(m, m, 70 + i)]
    return np.ascontiguousarray(np.vstack(parts))


@pytest.mark.parametrize("m", [64, 200])
def test_mixed_ranks_in_one_batch(dev, m):
    """zero, identity, reversed identity, all ones, every row twice, one non-zero column (the last) and products of inner dimension 1, m / 2
    and m - 1 between random matrices: the neighbours in a workgroup (m = 64: four waves) do not disturb each other, and the loop's trip
    count follows each matrix' own rank"""
    oranks = check_exact(dev, mixed_stack(m), m, m)
    zero, eye, rev, ones, twice, column, r1, rhalf, rmost = oranks[0:18:2]
    assert (zero, eye, rev, ones, column, r1) == (0, m, m, 1, 1, 1)
    assert 1 < twice <= (m + 1) // 2 and 1 < rhalf <= m // 2 and m // 2 < rmost <= m - 1


# ---- the limit: augmented stacks built on the device ------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,na,nb", [(64, 64, 1), (10, 10, 10), (64, 64, 64), (200, 200, 100), (100, 128, 300)])
def test_limit_on_concatenated_stacks(dev, m, na, nb):
    """[A | B] by gf2_concat_dev, elimination limited to A's columns: the augmented part follows, P = min(m, limit)"""
    import torch
    batch = 60
    a, b = g.random_words(batch * m, na, 80 + m), g.random_words(batch * m, nb, 81 + m)
    # a few singular A among them
    a[m:2 * m] = 0
    a[3 * m + 1] = a[3 * m]
    both = g.bits_to_words(np.hstack([g.words_to_bits(a, na), g.words_to_bits(b, nb)]))
    C = dev.concat(dev.DMat.from_words(a, na), dev.DMat.from_words(b, nb))
    P = min(m, na)
    tr, tp = ints(batch), ints(batch * P)
    dev.echelonize_batch(C, m, ncols_limit=na, ranks=tr.data_ptr(), pivots=tp.data_ptr())
    torch.cuda.synchronize()
    ref, oranks, opiv = reference(both, m, na + nb, True, na)
    assert opiv.shape == (batch, P) and oranks[1] == 0 and oranks[3] < m
    assert np.array_equal(tr.cpu().numpy(), oranks) and np.array_equal(tp.cpu().numpy().reshape(batch, P), opiv)
    assert np.array_equal(C.to_words()[:, :g.width(na + nb)], ref)


@pytest.mark.parametrize("m,ncols,limit", [(33, 100, 1), (200, 200, 1), (200, 200, 70), (64, 200, 70), (7, 5, 3), (300, 1000, 1000), (100, 100, 0)])
def test_limit_inside_the_matrix(dev, m, ncols, limit):
    """limit 1, a limit inside a word (70 of 200 columns), and limits that mean "all columns" (0, ncols)"""
    check_exact(dev, g.random_words(30 * m, ncols, 90 + m + limit), m, ncols, limit)


# ---- full = 0 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,ncols,limit", [(64, 64, 0), (40, 193, 0), (10, 10, 0), (200, 300, 0), (65, 64, 0), (64, 130, 64), (128, 256, 128)])
def test_upper_echelon_form(dev, m, ncols, limit):
    """full = 0: rank and pivot columns are those of the reduced form, row i starts at pivot column i with zeros below it, rows from the
    rank on are zero (inside the limit), and the reduced form of the result is the reduced form of the input (the same row operations
    reach the augmented part)"""
    batch = 40
    words = g.random_words(batch * m, ncols, 120 + m)
    words[m:2 * m] = 0
    words[2 * m:3 * m] = words[2 * m]  # rank 1
    got, ranks, piv = run_batch(dev, words, m, ncols, False, limit)
    ref, oranks, opiv = reference(words, m, ncols, True, limit)
    assert np.array_equal(ranks, oranks) and np.array_equal(piv, opiv)
    L = limit_of(ncols, limit)
    for b in range(batch):
        bits = g.words_to_bits(got[b * m:(b + 1) * m], ncols)[:, :L]
        r = ranks[b]
        assert not bits[r:].any(), b
        assert list(np.argmax(bits[:r], axis=1)) == list(piv[b, :r]) and bits[:r].any(axis=1).all(), b
        for i, c in enumerate(piv[b, :r]):
            assert not bits[i + 1:, c].any(), (b, i)
        again, rank2, _ = g.o_echelonize(got[b * m:(b + 1) * m], m, ncols, full=True, limit=limit)
        assert rank2 == r and np.array_equal(again, ref[b * m:(b + 1) * m]), b


# ---- views ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,ncols,batch,ld,cw0", [(64, 64, 9, 6, 2), (10, 100, 50, 8, 4), (64, 321, 6, 10, 2), (100, 130, 5, 6, 2), (300, 1000, 2, 20, 4),
                                                  (33, 130, 20, 7, 1), (64, 64, 5, 3, 1)])  # rows that are only 8-byte aligned
def test_views_keep_their_parent(dev, m, ncols, batch, ld, cw0):
    """A is a view at a column word offset and a row offset inside a buffer full of a poison word, its row stride larger than its
    width: after the call every word outside the view still holds the poison"""
    import torch
    w, r0, rows = g.width(ncols), 3, batch * m
    words = g.random_words(rows, ncols, 140 + m)
    parent = np.full((rows + 5, ld), POISON, dtype=np.uint64)
    parent[r0:r0 + rows, cw0:cw0 + w] = words
    t, tr, tp = to_gpu(parent), ints(batch), ints(batch * min(m, ncols))
    view = dev.DMat.wrap(t.data_ptr() + 8 * (r0 * ld + cw0), rows, ncols, ld, keep=t)
    dev.echelonize_batch(view, m, ranks=tr.data_ptr(), pivots=tp.data_ptr())
    torch.cuda.synchronize()
    ref, oranks, opiv = reference(words, m, ncols)
    expect = parent.copy()
    expect[r0:r0 + rows, cw0:cw0 + w] = ref
    assert np.array_equal(to_host(t), expect)
    assert np.array_equal(tr.cpu().numpy(), oranks) and np.array_equal(tp.cpu().numpy().reshape(opiv.shape), opiv)


@pytest.mark.parametrize("n", [40, 100])
def test_inverse_views_keep_their_parents(dev, n):
    """A and Ainv are views of ONE poisoned buffer, side by side: A and the poison around both are unchanged"""
    import torch
    batch, ld, w = 12, 8, g.width(n)
    words = g.random_words(batch * n, n, 150 + n)
    parent = np.full((batch * n + 2, ld), POISON, dtype=np.uint64)
    parent[1:1 + batch * n, 0:w] = words
    t, ts = to_gpu(parent), ints(batch)
    A = dev.DMat.wrap(t.data_ptr() + 8 * ld, batch * n, n, ld, keep=t)
    Ainv = dev.DMat.wrap(t.data_ptr() + 8 * (ld + 4), batch * n, n, ld, keep=t)
    # the two views interleave row by row: their address RANGES meet, which the call refuses (like the block copy with different ld)
    with pytest.raises(Exception, match="overlap"):
        dev.inverse_batch(A, n, Ainv=Ainv, singular=ts.data_ptr())
    # so Ainv is a view of a second poisoned buffer
    t2 = to_gpu(np.full((batch * n + 2, ld), POISON, dtype=np.uint64))
    Ainv = dev.DMat.wrap(t2.data_ptr() + 8 * (ld + 4), batch * n, n, ld, keep=t2)
    dev.inverse_batch(A, n, Ainv=Ainv, singular=ts.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(to_host(t), parent), "A or its surroundings changed"
    expect = np.full((batch * n + 2, ld), POISON, dtype=np.uint64)
    sing = np.zeros(batch, dtype=np.int32)
    for b in range(batch):
        inv = g.o_inverse(words[b * n:(b + 1) * n], n)
        sing[b] = inv is None
        if inv is not None:
            expect[1 + b * n:1 + (b + 1) * n, 4:4 + w] = inv
    assert 0 < sing.sum() < batch
    assert np.array_equal(ts.cpu().numpy(), sing) and np.array_equal(to_host(t2), expect)


# ---- offsets beyond 4 GiB -----------------------------------------------------------------------------------------------------------------

def test_offsets_beyond_4_gib(dev):
    """A view of 1040 matrices of 8 x 64 whose row stride is 65536 words, inside an allocation of 4.06 GiB: the byte offset of the last
    rows is beyond 2^32 (row 8191 is the last one below it), so a row offset computed in 32 bits lands in the wrong place.  Only the
    view is filled and read; the first, a middle and the last matrix are compared.  (A WORD index beyond 2^31 would take 16 GiB: that
    the kernels compute (b * m + r) * ld in 64 bits is left to reading gf2_elim_batch.hip.)"""
    import torch
    m, ncols, batch, ld = 8, 64, 1040, 65536
    rows = batch * m
    t = torch.empty(((rows - 1) * ld + 2,), dtype=torch.int64, device="cuda")
    assert t.numel() * 8 > (1 << 32) and (rows - 1) * ld * 8 > (1 << 32)
    words = g.random_words(rows, ncols, 160)
    col = t[: (rows - 1) * ld + 1: ld]  # word 0 of every row of the view
    assert col.numel() == rows
    col.copy_(torch.from_numpy(words[:, 0].view(np.int64).copy()).cuda())
    tr, tp = ints(batch), ints(batch * m)
    dev.echelonize_batch(dev.DMat.wrap(t.data_ptr(), rows, ncols, ld, keep=t), m, ranks=tr.data_ptr(), pivots=tp.data_ptr())
    torch.cuda.synchronize()
    got = col.cpu().numpy().view(np.uint64).reshape(rows, 1)
    ranks, piv = tr.cpu().numpy(), tp.cpu().numpy().reshape(batch, m)
    for b in (0, batch // 2, 1023, 1024, batch - 1):
        ref, orank, cols = g.o_echelonize(words[b * m:(b + 1) * m], m, ncols, full=True)
        assert np.array_equal(got[b * m:(b + 1) * m], ref), b
        assert ranks[b] == orank and list(piv[b, :orank]) == cols and (piv[b, orank:] == -1).all(), b


# ---- the inverse --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inverse_reference(n, batch):
    """(A, [inverse or None per matrix]); computed once, never written"""
    words = g.random_words(batch * n, n, 200 + n)
    words.setflags(write=False)
    return words, [g.o_inverse(words[b * n:(b + 1) * n], n) for b in range(batch)]


@pytest.mark.parametrize("n,batch", INVERSE_SIZES, ids=["%dx%d" % s for s in INVERSE_SIZES])
def test_inverse_batch(dev, n, batch):
    """Ainv and singular against o_inverse; Ainv holds poison before, and the blocks of singular matrices hold it afterwards; A is
    unchanged.  About 29 % of random matrices over GF(2) are invertible (50 % at n = 1): both classes are well represented."""
    import torch
    words, invs = inverse_reference(n, batch)
    good = sum(i is not None for i in invs)
    least = 32 if batch >= 256 else 1
    assert good >= least and batch - good >= least, (n, good)
    w, ld = g.width(n), padded(words).shape[1]
    ta, ti, ts = to_gpu(padded(words)), to_gpu(np.full((batch * n, ld), POISON, dtype=np.uint64)), ints(batch)
    dev.inverse_batch(dev.DMat.from_torch(ta, n), n, Ainv=dev.DMat.from_torch(ti, n), singular=ts.data_ptr())
    torch.cuda.synchronize()
    expect = np.full((batch * n, ld), POISON, dtype=np.uint64)
    for b, inv in enumerate(invs):
        if inv is not None:
            expect[b * n:(b + 1) * n, :w] = inv
    assert np.array_equal(ts.cpu().numpy(), np.array([i is None for i in invs], dtype=np.int32))
    bad = np.flatnonzero((to_host(ti) != expect).any(axis=1))
    assert bad.size == 0, (n, "first differing matrix", bad[0] // n, "row", bad[0] % n)
    assert np.array_equal(to_host(ta), padded(words)), "A changed"


# ---- stream order -------------------------------------------------------------------------------------------------------------------------

def as_words(int_array):
    """int32 values in the uint64 arrays the lanes carry (an even count)"""
    assert int_array.size % 2 == 0
    return np.ascontiguousarray(int_array.astype(np.int32)).view(np.uint64).reshape(1, -1)


def test_calls_are_asynchronous_and_ordered_on_their_streams(dev):
    """Two caller streams held back by a sleep.  Lane 0: echelonize_batch (full = 0) on a 64 x 64 stack, then a second call (full = 1)
    on its result; lane 1: inverse_batch on a 100 x 100 stack.  Inputs, ranks, pivot columns and singular flags are tensors that hold
    poison until the stream's own copy writes them behind the sleep, and torch ops on the same stream read them: a step that ran
    early, on another stream or on the host would see the poison or be overwritten by the copy.  run_pending checks that every call
    had returned while the streams were still held back."""
    m, batch, n, nb = 64, 64, 100, 16
    a = g.random_words(batch * m, m, 300)
    a[m:2 * m] = 0
    ref, oranks, opiv = reference(a, m, m)
    c = g.random_words(nb * n, n, 301)
    invs = [g.o_inverse(c[b * n:(b + 1) * n], n) for b in range(nb)]
    assert 0 < sum(i is None for i in invs) < nb
    stale = lambda count: as_words(np.full(count, INT_POISON))  # noqa: E731  what the arrays hold once the stream's copy has run
    lane0 = [padded(a), stale(batch), stale(batch * m), stale(batch), stale(batch * m)]
    lane1 = [padded(c), np.full((nb * n, 2), 7, dtype=np.uint64), stale(nb)]

    def issue(ls):
        t, s = ls[0].live, ls[0].handle
        A = dev.DMat.from_torch(t[0], m)
        dev.echelonize_batch(A, m, full=False, ranks=t[1].data_ptr(), pivots=t[2].data_ptr(), stream=s)
        dev.echelonize_batch(A, m, full=True, ranks=t[3].data_ptr(), pivots=t[4].data_ptr(), stream=s)
        t, s = ls[1].live, ls[1].handle
        dev.inverse_batch(dev.DMat.from_torch(t[0], n), n, Ainv=dev.DMat.from_torch(t[1], n), singular=t[2].data_ptr(), stream=s)

    def check(_, outs):
        ga, r1, p1, r2, p2 = outs[0]
        assert np.array_equal(ga[:, :1], ref)
        for r, p in ((r1, p1), (r2, p2)):  # the second call sees the first one's echelon form: same ranks, same pivot columns
            assert np.array_equal(r.view(np.int32).reshape(-1), oranks) and np.array_equal(p.view(np.int32).reshape(batch, m), opiv)
        gc, gi, gs = outs[1]
        assert np.array_equal(gc, padded(c)), "A changed"
        assert np.array_equal(gs.view(np.int32).reshape(-1), np.array([i is None for i in invs], dtype=np.int32))
        for b, inv in enumerate(invs):
            assert np.array_equal(gi[b * n:(b + 1) * n], inv if inv is not None else np.full((n, 2), 7, dtype=np.uint64)), b

    run_pending([lane0, lane1], issue, check)
