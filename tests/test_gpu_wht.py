"""GPU tests of include/m4ri_hip_wht.h: the Walsh-Hadamard transform against the plain butterfly loop of tests/wht_ref.py (itself checked
against the definition by tests/test_wht_reference.py), the LPN tally against numpy.bincount on the bits, the errors of all 2^k
secrets against the product route of INTEGRATION.md section 4 and against a brute-force count, and the minimum.

Which k take which path is read from gf2_wht_plan, never written down here.  Up to k = 18 the reference runs in numpy; above, the same
function runs on a torch tensor on the device (a numpy run of 2^28 int64 over 28 levels would take most of a minute, a case here a
few seconds at the most), after one case has compared the two at k = 18."""
import gc

import numpy as np
import pytest

import dirty_pool as dp
import gf2util as g
import limits_ref as lr
import wht_ref as wr
from census_util import assert_route, census
from stream_util import padded, run_pending

pytestmark = pytest.mark.gpu

SENT = 0x5EAD5EAD    # what an output holds before the call
NUMPY_MAX_K = 18     # the reference in numpy up to here, on the device above


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


@pytest.fixture(scope="module")
def L(pkg):
    return pkg._lib.lib()


def guarded(n):
    """n device ints on a 16-byte boundary between sentinels, all holding SENT; -> (tensor, address of the n ints)"""
    import torch
    t = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 16


def read_guarded(t):
    h = t.cpu().numpy()
    assert np.all(h[:4] == SENT) and np.all(h[-4:] == SENT), "a word next to the output was written"
    return h[4:-4]


def write_guarded(t, values):
    import torch
    t[4:-4] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).cuda()


# ---- the plan's boundaries -------------------------------------------------------------------------------------------------------

def plan_table(dev):
    return {k: dev.wht_plan(k) for k in range(31)}


def transform_ks(dev):
    """below and at a vector, a lane's registers, a wave; every tile length of the first pass (each leaves other lanes and levels out);
    around the first pass's levels B; every width a later pass can have; k_p - 1 and k_p for every pass count p (k_3 - 1 is the last k
    of two passes).  k = 30 has a test of its own."""
    P = plan_table(dev)
    B = P[30][1][1]
    ks = {0, 1, 2, 3, 5, 6, 7, B - 1, B, B + 1} | set(range(B + 1))
    first_k, width_k = {}, {}
    for k in range(31):
        passes, bounds = P[k][0], P[k][1]
        first_k.setdefault(passes, k)
        for p in range(1, passes):
            width_k.setdefault(bounds[p + 1] - bounds[p], k)
    for p, k in first_k.items():
        if p >= 2:
            ks |= {k - 1, k}
    ks |= set(width_k.values())
    assert max(first_k) == P[30][0] >= 3 and first_k[2] == B + 1
    return sorted(ks - {30}), first_k


def test_the_cases_cover_the_plan(dev):
    ks, first_k = transform_ks(dev)
    P = plan_table(dev)
    assert {P[k][0] for k in ks} | {P[30][0]} == set(range(max(first_k) + 1))      # every pass count
    widths = {b - a for k in range(31) for a, b in zip(P[k][1][1:], P[k][1][2:])}
    assert widths == {b - a for k in ks for a, b in zip(P[k][1][1:], P[k][1][2:])}   # every width of a later pass
    assert all(k - 1 in ks and k in ks for p, k in first_k.items() if p >= 2 and k < 30)
    assert max(ks) < 30 and len(ks) <= 24


def transform_cases():
    """(k,) cases need the plan, which needs the library: collected at import from the built library when there is one"""
    try:
        from m4ri_rust_amd import device
        return transform_ks(device)[0]
    except Exception:   # not built yet: the fixture builds; the fixed list is checked against the plan by the test above
        return list(range(19)) + [22, 23, 27, 28]


KS = transform_cases()


def test_the_case_list_is_the_plans(dev):
    assert KS == transform_ks(dev)[0]


# ---- the transform ---------------------------------------------------------------------------------------------------------------

def run_wht(dev, ptr, k):
    import torch
    torch.cuda.synchronize()
    assert dev.wht(ptr, k) is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", [k for k in KS if k <= NUMPY_MAX_K])
def test_transform_against_numpy(dev, k):
    n = 1 << k
    rng = np.random.default_rng(500 + k)
    s = np.arange(n, dtype=np.int64)
    v1, v2 = int(rng.integers(0, n)), int(rng.integers(0, n))
    rand = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64)
    inputs = {"random": rand, "ones": np.ones(n, dtype=np.int64), "+1": np.where(s == v1, 1, 0), "-1": np.where(s == v2, -1, 0)}
    closed = {"ones": np.where(s == 0, n, 0), "+1": wr.delta_transform(s, v1, 1, k), "-1": wr.delta_transform(s, v2, -1, k)}
    for name, f in inputs.items():
        t, p = guarded(n)
        write_guarded(t, wr.as_int32(f & wr.MASK))
        run_wht(dev, p, k)
        got = read_guarded(t)
        want = wr.wht_reference(f, k)
        assert np.array_equal(got, wr.as_int32(want)), (k, name, np.flatnonzero(got != wr.as_int32(want))[:8])
        if name in closed:
            assert np.array_equal(got, wr.as_int32(closed[name] & wr.MASK)), (k, name)
        run_wht(dev, p, k)   # twice the transform is f << k
        assert np.array_equal(read_guarded(t), wr.as_int32((f << k) & wr.MASK)), (k, name, "twice")
    # the wrapper that uploads
    assert np.array_equal(dev.wht(wr.as_int32(rand & wr.MASK), k), wr.as_int32(wr.wht_reference(rand, k)))


def test_the_reference_on_the_device_is_the_numpy_reference():
    import torch
    k = NUMPY_MAX_K
    f = np.random.default_rng(1).integers(-(1 << 31), 1 << 31, 1 << k, dtype=np.int64)
    assert np.array_equal(wr.wht_reference(torch.from_numpy(f).cuda(), k).cpu().numpy(), wr.wht_reference(f, k))


@pytest.mark.parametrize("k", [k for k in KS if k > NUMPY_MAX_K])
def test_transform_against_the_reference_on_the_device(dev, L, k):
    import torch
    n = 1 << k
    gen = torch.Generator(device="cuda").manual_seed(900 + k)
    f64 = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=gen)
    f = (f64 - ((f64 >> 31) << 32)).to(torch.int32)   # the int32 with the same bits
    assert torch.equal(f.to(torch.int64) & wr.MASK, f64) and f.data_ptr() % 16 == 0
    want = wr.wht_reference(f64, k)
    run_wht(dev, f.data_ptr(), k)
    assert torch.equal(f.to(torch.int64) & wr.MASK, want), (k, "random")
    del want
    run_wht(dev, f.data_ptr(), k)
    assert torch.equal(f.to(torch.int64) & wr.MASK, (f64 << k) & wr.MASK), (k, "twice")
    del f64
    f.fill_(1)
    run_wht(dev, f.data_ptr(), k)
    assert int(f[0]) == n and not bool(f[1:].any()), (k, "ones")
    s = torch.arange(n, dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(k)
    for sign in (1, -1):
        v = int(rng.integers(0, n))
        f.zero_()
        f[v] = sign
        run_wht(dev, f.data_ptr(), k)
        assert torch.equal(f.to(torch.int64), wr.delta_transform(s, v, sign, k)), (k, sign, v)
    del f, s
    gc.collect()
    torch.cuda.empty_cache()


def test_transform_of_2_to_30(dev, L):
    """the array is exactly 2^32 bytes, where a 32-bit byte offset wraps, and the plan has its largest pass count: a handful of +-1
    entries against their closed form F[s] = sum of sign_i (-1)^<s, v_i>, computed with torch on the device in chunks"""
    import torch
    k, n = 30, 1 << 30
    assert dev.wht_plan(k)[0] == max(dev.wht_plan(j)[0] for j in range(31))
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    rng = np.random.default_rng(30)
    entries = [(0, 1), (n - 1, -1), ((1 << 29) + 12345, 1), (int(rng.integers(0, n)), -1), (int(rng.integers(n // 2, n)), 1)]
    f = torch.zeros(n, dtype=torch.int32, device="cuda")
    for v, sign in entries:
        f[v] = sign
    run_wht(dev, f.data_ptr(), k)
    chunk = 1 << 26
    for s0 in range(0, n, chunk):
        s = torch.arange(s0, s0 + chunk, dtype=torch.int64, device="cuda")
        want = sum(wr.delta_transform(s, v, sign, k) for v, sign in entries)
        assert torch.equal(f[s0:s0 + chunk].to(torch.int64), want), s0
    del f, s, want
    gc.collect()
    torch.cuda.empty_cache()


# ---- the tally -------------------------------------------------------------------------------------------------------------------

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


class Operand:
    """`words` (nrows x width(ncols)) on the device: a buffer of its own, or (view) rows of a parent that holds ones in every other
    bit -- the words before, between and behind the rows, the excess bits of the last word -- with an odd ld at an odd word"""

    def __init__(self, dev, words, ncols, view):
        nrows, w = words.shape
        if view:
            ld = w + 3 if (w + 3) & 1 else w + 4
            r0, c0 = 1, 2                       # word r0 * ld + c0 of the parent: odd
            self.host = np.full((nrows + 3, ld), ONES, dtype=np.uint64)
            words = words.copy()
            if ncols % 64 and nrows:
                words[:, -1] |= ~np.uint64((1 << (ncols % 64)) - 1)
        else:
            ld = max((w + 1) & ~1, 1)
            r0, c0 = 0, 0
            self.host = np.zeros((max(nrows, 1), ld), dtype=np.uint64)[:nrows]
        self.host[r0:r0 + nrows, c0:c0 + w] = words
        import torch
        self.t = torch.from_numpy(self.host.view(np.int64).copy()).cuda() if self.host.size else None
        base = self.t.data_ptr() if self.t is not None else 0
        assert not view or ((ld & 1) and ((r0 * ld + c0) & 1))
        self.m = dev.DMat.wrap(base + 8 * (r0 * ld + c0) if base else 0, nrows, ncols, ld, keep=self.t)

    def unchanged(self):
        if self.t is not None:
            assert np.array_equal(self.t.cpu().numpy().view(np.uint64).reshape(self.host.shape), self.host), "the operand changed"


def indices_and_labels(words, ncols, c0, k, label):
    bits = g.words_to_bits(words, ncols) if words.shape[0] else np.zeros((0, ncols), dtype=np.uint8)
    idx = np.zeros(words.shape[0], dtype=np.int64)
    for j in range(k):
        idx |= bits[:, c0 + j].astype(np.int64) << j
    lab = bits[:, label].astype(np.int64) if label >= 0 else np.zeros(words.shape[0], dtype=np.int64)
    return idx, lab


def tally_by_bincount(words, ncols, c0, k, label):
    idx, lab = indices_and_labels(words, ncols, c0, k, label)
    n = 1 << k
    return np.bincount(idx[lab == 0], minlength=n) - np.bincount(idx[lab == 1], minlength=n)


def device_tally(dev, M, c0, k, label):
    import torch
    t, p = guarded(1 << k)
    torch.cuda.synchronize()
    assert dev.lpn_tally(M, c0, k, label, out=p + 0) is None
    torch.cuda.synchronize()
    return read_guarded(t)


def variant_change(dev):
    """the first k whose tally adds straight into f"""
    vs = [dev.wht_plan(k)[4] for k in range(31)]
    return vs.index(1)


# (nrows, ncols, c0, k, label): k None -> the last LDS-histogram k, "g" -> the first global-atomic k
TALLY_CASES = [
    (0, 200, 37, 10, 3),
    (1, 200, 0, 10, 150),          # the label in another word than the index
    (63, 200, 37, 10, 40),         # the label inside the index range
    (65, 200, 50, 20, -1),         # the range straddles a word; no label
    (65, 200, 50, 20, 60),         # ... with the label in the range's first word
    (1000, 200, 184, 16, 5),       # c0 + k == ncols, ncols no multiple of 64, the range straddles
    (1000, 70, 64, 6, 3),          # the whole range in the short last word
    (1000, 256, 192, None, 255),   # the last column is the label
    (100003, 256, 37, None, 255),
    (100003, 256, 50, "g", 0),
    (100003, 130, -1, "g", 129),   # c0 = ncols - k: the range straddles, ends at ncols and holds the label
    (100003, 64, 0, 0, 63),        # no index bit: f[0] = label 0 rows - label 1 rows
    (5, 64, 64, 0, -1),            # c0 == ncols: f[0] = nrows
]


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("case", TALLY_CASES, ids=lambda c: "%dx%d-c%d-k%s-l%d" % c)
def test_tally(dev, L, case, view):
    nrows, ncols, c0, k, label = case
    kv = variant_change(dev)
    k = kv - 1 if k is None else kv if k == "g" else k
    if c0 < 0:
        c0 = ncols - k
        assert c0 % 64 + k > 64 and c0 <= label
    words = g.random_words(nrows, ncols, 7 * nrows + c0 + k)
    op = Operand(dev, words, ncols, view)
    k0 = census(L)
    got = device_tally(dev, op.m, c0, k, label)
    want = tally_by_bincount(words, ncols, c0, k, label)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert int(np.abs(got.astype(np.int64)).sum()) <= nrows and (label >= 0 or int(got.sum()) == nrows)
    if nrows:
        assert_route(k0, census(L), ["gf2_wht_tally_kernelILb%d" % (1 if k < kv else 0)])
    op.unchanged()


def test_tally_of_identical_rows(dev, L):
    """100 003 equal rows: every add lands on one counter, in LDS and in global memory"""
    nrows, ncols, c0 = 100003, 200, 50
    kv = variant_change(dev)
    row = g.random_words(1, ncols, 99)
    words = np.repeat(row, nrows, axis=0)
    for k, label in ((10, 3), (kv - 1, 190), (kv, 190), (20, -1)):
        idx, lab = indices_and_labels(row, ncols, c0, k, label)
        got = device_tally(dev, Operand(dev, words, ncols, False).m, c0, k, label)
        want = np.zeros(1 << k, dtype=np.int64)
        want[idx[0]] = -nrows if lab[0] else nrows
        assert np.array_equal(got, want), (k, label)


def test_wrapper_returns_numpy(dev):
    words = g.random_words(1000, 200, 5)
    P = dev.DMat.from_words(words, 200)
    assert np.array_equal(dev.lpn_tally(P, 37, 9, 150), tally_by_bincount(words, 200, 37, 9, 150))
    assert np.array_equal(dev.lpn_tally(P, 37, 9), tally_by_bincount(words, 200, 37, 9, -1))


def test_tally_of_an_operand_past_4gib(dev, L):
    """8 400 000 x 4096 (4.3 GB) filled by gf2_dmat_fill_random: the index straddles the last two words of a row, the label is the last
    column; the expected counts come from torch on the device"""
    import ctypes
    import torch
    m, n, seed = 8_400_000, 4096, 0x7A11
    c0, k, label = 62 * 64 + 56, 16, 4095
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((m, 64), dtype=torch.int64, device="cuda")
    A = dev.DMat.from_torch(t, n)
    assert m * A.ld * 8 > lr.LIMIT_BYTES
    dev._lib.check(L.gf2_dmat_fill_random(ctypes.byref(A.s), seed, None), "gf2_dmat_fill_random")
    torch.cuda.synchronize()
    picks = np.array([0, m - 1] + list(lr.straddle(A.ld, m)))
    assert np.array_equal(t[torch.from_numpy(picks).cuda()].cpu().numpy().view(np.uint64), lr.seeded_words(seed, n, picks))
    w62, w63 = t[:, 62], t[:, 63]
    idx = ((w62 >> 56) & 0xFF) | ((w63 & 0xFF) << 8)
    lab = w63 < 0   # bit 63
    want = torch.bincount(idx[~lab], minlength=1 << k) - torch.bincount(idx[lab], minlength=1 << k)
    got, p = guarded(1 << k)
    torch.cuda.synchronize()
    dev.lpn_tally(A, c0, k, label, out=p)
    torch.cuda.synchronize()
    got = read_guarded(got)
    assert np.array_equal(got, want.cpu().numpy())
    assert int(got.sum()) == m - 2 * int(lab.sum()) and int(np.abs(got).sum()) <= m
    # the rows behind byte offset 2^32 alone, as a view: their counts are what is missing from the rows before
    r0 = lr.straddle(A.ld, m)[1]
    late = torch.bincount(idx[r0:][~lab[r0:]], minlength=1 << k) - torch.bincount(idx[r0:][lab[r0:]], minlength=1 << k)
    early = device_tally(dev, lr.row_view(dev, A, 0, r0), c0, k, label)
    assert np.array_equal(got - early, late.cpu().numpy())
    del t, A, w62, w63, idx, lab
    gc.collect()
    torch.cuda.empty_cache()


# ---- the errors ------------------------------------------------------------------------------------------------------------------

def lpn_pool(N, k, tau, seed, ncols=None, c0=0, label=None):
    """N samples of k bits at columns [c0, c0 + k) of random rows, labels <sample, secret> + noise at column `label` -> (words, ncols,
    secret index, noise weight)"""
    rng = np.random.default_rng(seed)
    ncols = k + 1 if ncols is None else ncols
    label = k if label is None else label
    bits = rng.integers(0, 2, (N, ncols), dtype=np.uint8)
    secret = rng.integers(0, 2, k, dtype=np.uint8)
    noise = (rng.random(N) < tau).astype(np.uint8)
    bits[:, label] = (bits[:, c0:c0 + k].astype(np.int64) @ secret.astype(np.int64) + noise) % 2
    return g.bits_to_words(bits), ncols, int(sum(int(b) << j for j, b in enumerate(secret))), int(noise.sum())


@pytest.mark.parametrize("k", [8, 12])
def test_errors_are_the_column_weights_of_the_product(dev, k):
    """the identity INTEGRATION.md section 4 promises: errors == col_weights(pool * [S ; 1]) for S = all 2^k vectors"""
    N = 10007
    words, ncols, _, _ = lpn_pool(N, k, 0.125, 40 + k)
    pool = dev.DMat.from_words(words, ncols)
    s1 = np.ones((k + 1, 1 << k), dtype=np.uint8)
    for j in range(k):
        s1[j] = (np.arange(1 << k) >> j) & 1
    S1 = dev.DMat.from_words(g.bits_to_words(s1), 1 << k)
    want = dev.col_weights(dev.mul(pool, S1))
    got = pool.lpn_errors(0, k, k)
    assert got.dtype == np.int32 and np.array_equal(got, want)


@pytest.mark.parametrize("view", [False, True], ids=["plain", "view"])
@pytest.mark.parametrize("k", [0, 1, 2, 5, 10])
def test_errors_against_brute_force(dev, k, view):
    N, ncols, c0, label = 1000, 200, 57, 130
    words, _, _, _ = lpn_pool(N, k, 0.25, 70 + k, ncols, c0, label)
    idx, lab = indices_and_labels(words, ncols, c0, k, label)
    s = np.arange(1 << k, dtype=np.int64)
    want = (wr.parity(idx[:, None] & s[None, :], max(k, 1)) != lab[:, None]).sum(axis=0)
    op = Operand(dev, words, ncols, view)
    import torch
    t, p = guarded(1 << k)
    torch.cuda.synchronize()
    assert dev.lpn_errors(op.m, c0, k, label, out=p) is None
    torch.cuda.synchronize()
    assert np.array_equal(read_guarded(t), want)
    op.unchanged()
    # no sample, nobody wrong
    t, p = guarded(1 << k)
    dev.lpn_errors(Operand(dev, words[:0], ncols, view).m, c0, k, label, out=p)
    torch.cuda.synchronize()
    assert not read_guarded(t).any()


def test_planted_secret(dev):
    """tau = 1/8, N = 2^16, k = 16: the minimum is the secret, its error count the planted noise weight exactly, and the selection with
    the window [0, that count] returns that index alone -- all on device arrays"""
    import torch
    N, k = 1 << 16, 16
    words, ncols, secret, weight = lpn_pool(N, k, 0.125, 2026)
    pool = dev.DMat.from_words(words, ncols)
    errors, pe = guarded(1 << k)
    out, po = guarded(4)     # idx of the minimum, its value, the selection's count, the selected index
    torch.cuda.synchronize()
    dev.lpn_errors(pool, 0, k, k, out=pe)
    dev.min_weight(pe, 1 << k, idx=po, val=po + 4)
    torch.cuda.synchronize()
    idx, val = (int(x) for x in read_guarded(out)[:2])
    assert idx == secret and val == weight
    dev.select_weights(pe, 1 << k, 0, val, idx=po + 12, cap=1, count=po + 8)
    torch.cuda.synchronize()
    assert list(read_guarded(out)) == [secret, weight, 1, secret]
    e = read_guarded(errors)
    assert e[secret] == weight and np.all(np.delete(e, secret) > N // 4)


# ---- the minimum -----------------------------------------------------------------------------------------------------------------

def lowest_argmin(w):
    return int(np.flatnonzero(w == w.min())[0]), int(w.min())


@pytest.mark.parametrize("n", [1, 2, 63, 1023, 1024, 1025, 100003, (1 << 20) + 77, (1 << 21) + 5])
def test_min(dev, n):
    """n below, at and above a block and above what the grid covers in one sweep; ties, the last element, negative values"""
    import torch
    rng = np.random.default_rng(n)
    block, groups = 1024, dev.wht_plan(30)[5] // 8   # a pair of ints per workgroup
    cases = {
        "ties": rng.integers(-5, 50, n),
        "last": np.concatenate([rng.integers(10, 1 << 30, n - 1), [3]]),
        "negative": rng.integers(-(1 << 31), -(1 << 30), n),
        "equal": np.full(n, (1 << 31) - 1),
        "tie across workgroups": np.where(np.arange(n) % (block * 3 + 1) == block + 7, -9, rng.integers(0, 9, n)),
    }
    if n > block * groups:
        tail = rng.integers(5, 100, n)
        tail[block * groups + 1] = 4   # reached only by a workgroup's second sweep
        cases["second sweep"] = tail
    for name, w in cases.items():
        w = np.asarray(w, dtype=np.int64)
        tw, pw = guarded(n)
        write_guarded(tw, w)
        out, po = guarded(2)
        torch.cuda.synchronize()
        assert dev.min_weight(pw, n, idx=po, val=po + 4) == (None, None)
        torch.cuda.synchronize()
        assert tuple(read_guarded(out)) == lowest_argmin(w), (n, name)
        assert np.array_equal(read_guarded(tw), w)
        if n > 1:   # from the second value on: off a 16-byte boundary, where the kernel loads single values
            out, po = guarded(2)
            dev.min_weight(pw + 4, n - 1, idx=po, val=po + 4)
            torch.cuda.synchronize()
            assert tuple(read_guarded(out)) == lowest_argmin(w[1:]), (n, name, "unaligned")
    w = cases["ties"]
    assert dev.min_weight(w, n) == lowest_argmin(np.asarray(w))


def test_min_on_dirty_scratch(dev, L):
    """the per-workgroup minima come from a cache in which every block holds a pattern (as pairs of ints: (1, 1), or random bits), no
    block comes fresh from the driver, and every value of the array lies above 1: a partial read without having been written wins"""
    import torch
    rng = np.random.default_rng(11)
    for pattern in dp.PATTERNS:
        pool = dp.Pool(L, pattern)
        for n in (3000, 100003):
            w = rng.integers(100, 1 << 30, n)
            w[n - 5] = w[n // 2] = 50
            stream = torch.cuda.Stream().cuda_stream   # a caller stream: its arena is new
            h0, k0 = pool.hits(), census(L)
            got = dev.min_weight(w, n, stream=stream)
            assert pool.hits() - h0 >= 1
            assert got == (n // 2, 50), (pattern, n, got)
            assert_route(k0, census(L), ["gf2_wht_min_partial_kernel", "gf2_wht_min_fold_kernel"])
            pool.no_fresh("the minimum on dirty scratch")
    gc.collect()
    L.gf2_trim()


# ---- stream order ----------------------------------------------------------------------------------------------------------------

def packed_ints(count, fill=0):
    return np.full((1, (count + 1) // 2), np.uint64(fill), dtype=np.uint64)


def test_behind_pending_work_on_a_caller_stream(dev):
    """the pool is written by a copy that waits behind a sleep on the caller's stream; tally -> transform -> select, and errors ->
    minimum -> select, are enqueued behind it before anything synchronises.  A step on another stream, or a wait on the host, would see
    the poison."""
    N = 5000
    k = dev.wht_plan(30)[1][1] + 1    # two passes
    words, ncols, secret, weight = lpn_pool(N, k, 0.125, 77, ncols=100, c0=41, label=3)
    n = 1 << k
    f = tally_by_bincount(words, ncols, 41, k, 3)
    F = wr.as_int32(wr.wht_reference(f.astype(np.int64), k)).astype(np.int64)
    lo, hi = int(np.sort(F)[-5]), int(F.max())
    hits = np.flatnonzero((F >= lo) & (F <= hi))
    cap = len(hits) + 3
    assert F[secret] == N - 2 * weight == hi

    def issue(ls):
        (lane,) = ls
        tp, tf, ti, tn, te, tm = lane.live
        P = dev.DMat.wrap(tp.data_ptr(), N, ncols, tp.shape[1], keep=tp)
        s = lane.handle
        dev.lpn_tally(P, 41, k, 3, out=tf.data_ptr(), stream=s)
        dev.wht(tf.data_ptr(), k, stream=s)
        dev.select_weights(tf.data_ptr(), n, lo, hi, idx=ti.data_ptr(), cap=cap, count=tn.data_ptr(), stream=s)
        dev.lpn_errors(P, 41, k, 3, out=te.data_ptr(), stream=s)
        dev.min_weight(te.data_ptr(), n, idx=tm.data_ptr(), val=tm.data_ptr() + 4, stream=s)
        dev.select_weights(te.data_ptr(), n, 0, weight, idx=tm.data_ptr() + 8, cap=1, count=tm.data_ptr() + 12, stream=s)

    def check(_, reads):
        ((rp, rf, ri, rn, re, rm),) = reads
        assert np.array_equal(rf.view(np.int32).reshape(-1)[:n], F)
        assert int(rn.view(np.int32).reshape(-1)[0]) == len(hits)
        assert np.array_equal(ri.view(np.int32).reshape(-1)[:len(hits)], hits)
        assert np.array_equal(re.view(np.int32).reshape(-1)[:n], (N - F) // 2)
        assert list(rm.view(np.int32).reshape(-1)[:4]) == [secret, weight, secret, 1]
        assert np.array_equal(rp[:, :words.shape[1]], words)

    run_pending([[padded(words), packed_ints(n), packed_ints(cap + (cap & 1)), packed_ints(2), packed_ints(n), packed_ints(4)]], issue, check)
