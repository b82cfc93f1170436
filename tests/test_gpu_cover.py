"""GPU tests of include/m4ri_hip_cover.h: gf2_cover_reduce_dev bit for bit against the numpy reduction of tests/cover_ref.py (itself
checked against full enumeration and a loop over bits by tests/test_cover_reference.py): every word of D's parent, dist between its
sentinels, and P afterwards.

Every operand of run() is a window of a dirty parent: random bits in every word of the parent -- the rows before and behind the window,
the words left and right of it, the excess bits of P's last word -- and the whole parent of D is compared afterwards, so a store outside
the rows' words, or an excess bit that is not zero, fails the case.  dist lies between sentinels and holds a pattern before the call.

Which kernel a case runs (0: rows read from global memory, 1: window words staged in LDS), the rows of a pass and the most workgroups
are read from gf2_cover_plan, never written down here; which kernel ran is read from the launch census."""
import gc

import numpy as np
import pytest

import cover_ref as cr
import gf2util as g
import lf1_ref as lf
import limits_ref as lr
import stream_util as su
import wht_ref as wr
from census_util import assert_route, census

pytestmark = pytest.mark.gpu

SENT = 0x5EAD5EAD    # what an int output holds before the call

# (ld odd, base on an odd word): 16-byte accesses are possible only with both even
EE, EO, OE, OO = (False, False), (False, True), (True, False), (True, True)
LAYOUT_PAIRS = [(EE, EE), (EE, OO), (OO, EE), (EO, OE), (OE, EO)]   # (P, D): every layout on either side, 16 bytes on both, one, none

GOLAY, HAM3, HAM4, HAM5, REP3, REP13, ID1, ID32, DROP12 = (cr.golay23(), cr.hamming(3), cr.hamming(4), cr.hamming(5), cr.repetition(3),
                                                           cr.repetition(13), cr.identity(1), cr.identity(32), cr.drop(12))
LIST = [GOLAY, HAM3, REP3, ID1, DROP12, HAM5, REP13, ID32, HAM4]     # 137 bits, 88 message bits


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
    """n device ints between sentinels, all holding SENT; -> (tensor, address of the n ints)"""
    import torch
    t = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
    return t, t.data_ptr() + 16


def read_guarded(t):
    h = t.cpu().numpy()
    assert np.all(h[:4] == SENT) and np.all(h[-4:] == SENT), "a word next to an int output was written"
    return h[4:-4]


def random_systematic(n, k, seed):
    rng = np.random.default_rng(seed)
    return cr.Code(n, k, tuple(int(rng.integers(0, 1 << k)) | 1 << (k + t) for t in range(n - k)))


_DEVICE_CODES = {}


def to_dev(dev, code, table=None):
    """the device.CoverCode of a reference code (and of a table of the caller's); kept, so that a table is uploaded once"""
    key = (code, None if table is None else table.tobytes())
    if key not in _DEVICE_CODES:
        _DEVICE_CODES[key] = dev.CoverCode.from_rows(code.n, code.k, code.h, table=table)
    return _DEVICE_CODES[key]


def plan_of(dev, nrows, ncols, segments):
    return dev.cover_plan(nrows, ncols, [to_dev(dev, c) for c in segments])


def R_of(dev):
    return plan_of(dev, 1000, 256, [GOLAY])[3]


def most_groups(dev):
    return plan_of(dev, 1 << 30, 256, [GOLAY])[8]


class View:
    """nrows x ncols as a window of a parent that holds random bits in every word; `words` (clean) go into the window, the excess
    bits of the last word stay dirty"""

    def __init__(self, dev, nrows, ncols, layout, seed, words=None):
        import torch
        ld_odd, base_odd = layout
        w = g.width(ncols)
        ld = w + 3
        if bool(ld & 1) != ld_odd:
            ld += 1
        r0 = 1
        cw = 1 if bool((r0 * ld + 1) & 1) == base_odd else 2
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 1 << 64, (nrows + 3, ld), dtype=np.uint64)
        self.r0, self.cw, self.w, self.ncols = r0, cw, w, ncols
        if words is not None and nrows and w:
            dirty = self.host[r0:r0 + nrows, cw:cw + w].copy()
            self.host[r0:r0 + nrows, cw:cw + w] = words
            if ncols % 64:
                self.host[r0:r0 + nrows, cw + w - 1] |= dirty[:, -1] & ~np.uint64((1 << (ncols % 64)) - 1)
        self.t = torch.from_numpy(self.host.view(np.int64).copy()).cuda()
        assert self.t.data_ptr() % 16 == 0 and bool(ld & 1) == ld_odd and bool((r0 * ld + cw) & 1) == base_odd
        self.m = dev.DMat.wrap(self.t.data_ptr() + 8 * (r0 * ld + cw), nrows, ncols, ld, keep=self.t)

    def read(self):
        return self.t.cpu().numpy().view(np.uint64).reshape(self.host.shape)

    def unchanged(self):
        assert np.array_equal(self.read(), self.host), "the operand changed"

    def with_rows(self, rows):
        """the parent as it must look after the rows of the window were written as whole rows"""
        want = self.host.copy()
        want[self.r0:self.r0 + len(rows), self.cw:self.cw + self.w] = rows
        return want


def run(dev, L, words, ncols, c0, segments, with_dist=True, layouts=(EE, EE), stream=None, tables=None, variant=None):
    """one gf2_cover_reduce_dev call on dirty windows against the reference -> (D words, dist) of the reference"""
    import torch
    N = words.shape[0]
    want_D, want_dist = cr.reduce(words, c0, segments, tables)
    K = sum(c.k for c in segments)
    dsegs = [to_dev(dev, c, None if tables is None else tables[j]) for j, c in enumerate(segments)]
    for code in dsegs:
        code.table_ptr()                               # uploaded ahead of the call
    P = View(dev, N, ncols, layouts[0], 11 * N + c0, words)
    D = View(dev, N, K, layouts[1], 13 * N + K)
    td, pd = guarded(max(N, 1))
    torch.cuda.synchronize()
    k0 = census(L)
    out = dev.cover_reduce(P.m, c0, dsegs, D=D.m, dist=pd if with_dist else dev.SKIP, stream=stream)
    assert out[0] is D.m and out[1] is None
    torch.cuda.synchronize()
    what = (N, ncols, c0, len(segments), K, layouts, with_dist)
    got = D.read()
    exp = D.with_rows(want_D)
    assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:8])
    d = read_guarded(td)
    if with_dist:
        assert np.array_equal(d[:N], want_dist), (what, np.flatnonzero(d[:N] != want_dist)[:8])
    assert np.all(d[N if with_dist else 0:] == SENT), what            # a NULL dist: nothing is written
    P.unchanged()
    plan = dev.cover_plan(N, ncols, dsegs)
    assert plan is not None and (variant is None or plan[0] == variant), (what, plan)
    if N and (K or with_dist):
        assert_route(k0, census(L), ["gf2_cover_kernelILb%d" % plan[0]])
    else:
        assert census(L) == k0, "nothing to write, and yet a kernel was launched"
    return want_D, want_dist


# ---- windows ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_dist", [True, False], ids=["dist", "nodist"])
@pytest.mark.parametrize("reverse", [False, True], ids=["list", "reversed"])
@pytest.mark.parametrize("c0", [0, 37, 63, 64])
def test_windows(dev, L, c0, reverse, with_dist):
    """blocks and messages straddle word boundaries at both ends"""
    segments = LIST[::-1] if reverse else LIST
    words = g.random_words(1000, 300, 100 + c0)
    want_D, want_dist = run(dev, L, words, 300, c0, segments, with_dist, layouts=(OO, EE) if reverse else (EE, OE))
    assert want_D.shape == (1000, 2) and 0 < want_dist.min() and want_dist.max() <= 12 + 1 + 1 + 1 + 6 + 1 + 3


# ---- the limits of the contract --------------------------------------------------------------------------------------------------------

def test_256_segments_of_8_codes(dev, L):
    eight = [HAM3, REP3, ID1, cr.drop(2), GOLAY, HAM4, cr.repetition(5), cr.identity(5)]
    segments = eight * 32
    assert len(segments) == 256 and len(set(segments)) == 8
    bits = sum(c.n for c in segments)
    words = g.random_words(300, bits + 40, 8)
    run(dev, L, words, bits + 40, 40, segments, layouts=(OE, OO), variant=0)
    run(dev, L, words, bits + 40, 0, segments[::-1], with_dist=False, layouts=(EE, EE))
    # ... and of the most codes a call takes
    sixteen = eight + [cr.identity(2), cr.identity(32), cr.drop(3), cr.drop(1), cr.repetition(4), cr.repetition(6), HAM5, DROP12]
    segments = sixteen * 16
    assert len(segments) == 256 and len(set(segments)) == 16 and plan_of(dev, 300, 8192, sixteen + [REP13]) is None
    bits = sum(c.n for c in segments)
    words = g.random_words(300, bits + 3, 16)
    run(dev, L, words, bits + 3, 3, segments, layouts=(EO, OE), variant=0)


def test_16384_table_words(dev, L):
    """four tables of 2^12 words: 64 KiB of tables in LDS, beside the staged rows"""
    four = [REP13, random_systematic(20, 8, 1), random_systematic(24, 12, 2), random_systematic(14, 2, 3)]
    assert plan_of(dev, 700, 200, four)[7] == 16384 and plan_of(dev, 700, 200, four)[2] > 65536
    assert plan_of(dev, 700, 200, four + [HAM3]) is None
    words = g.random_words(700, 200, 16384)
    run(dev, L, words, 200, 61, four, layouts=(EO, EE), variant=1)
    wide = g.random_words(300, 64 * 15, 16385)                      # and with the rows read from global memory
    run(dev, L, wide, 64 * 15, 3, (four + [ID32] * 4) * 3 + [ID32] * 10, layouts=(EE, OO), variant=0)


@pytest.mark.parametrize("case", [("K64", [ID32, ID32], 17), ("K128", [ID32] * 4, 64), ("K192", [ID32] * 6, 31),
                                  ("K270", [ID32, GOLAY, HAM5, ID32, ID32, REP3] * 2, 5),
                                  ("K1", [REP3], 62), ("K1-drop", [DROP12, REP13, DROP12], 50), ("id32-c33", [ID32], 33),
                                  ("id32-c32", [ID32], 32), ("id32-c0", [ID32], 0)], ids=lambda c: c[0])
def test_message_widths(dev, L, case):
    _, segments, c0 = case
    ncols = c0 + sum(c.n for c in segments) + (0 if c0 % 2 else 9)      # also a window that ends with the row
    words = g.random_words(777, ncols, c0)
    for layouts in ((EE, EE), (OO, OO)):
        want_D, want_dist = run(dev, L, words, ncols, c0, segments, layouts=layouts)
    if all(c.k == c.n for c in segments):
        assert not want_dist.any()


def test_no_message_bit_and_no_segment(dev, L):
    """K == 0 and nseg == 0: D has no column and only dist is written; without dist nothing is launched"""
    words = g.random_words(500, 130, 3)
    want_D, want_dist = run(dev, L, words, 130, 60, [DROP12, cr.drop(32), cr.drop(1)])
    assert want_D.shape == (500, 0) and np.array_equal(want_dist, cr.popcount(cr.blocks(words, 60, 32)) + cr.popcount(cr.blocks(words, 92, 13)))
    run(dev, L, words, 130, 60, [DROP12, cr.drop(32), cr.drop(1)], with_dist=False)
    want_D, want_dist = run(dev, L, words, 130, 130, [])
    assert not want_dist.any()
    run(dev, L, words, 130, 0, [], with_dist=False)
    # the wrapper sizes D and dist itself
    P = dev.DMat.from_words(words, 130)
    D, dist = dev.cover_reduce(P, 60, [dev.CoverCode.drop(12)])
    assert (D.nrows, D.ncols) == (500, 0) and np.array_equal(dist.read(None), cr.popcount(cr.blocks(words, 60, 12)))


def test_a_table_that_is_no_leader_table_is_taken_as_it_is(dev, L):
    code = random_systematic(20, 10, 2010)
    rng = np.random.default_rng(2010)
    table = rng.integers(0, 1 << 32, 1 << 10, dtype=np.uint32)        # random words, bits above n included
    words = g.random_words(900, 100, 2010)
    segments, tables = [ID1, code, HAM3, code], [None, table, None, table]
    want_D, want_dist = run(dev, L, words, 100, 41, segments, layouts=(OE, EE), tables=tables)
    honest_D, honest_dist = cr.reduce(words, 41, segments)
    assert not np.array_equal(want_D, honest_D) and want_dist.mean() > honest_dist.mean() + 5


# ---- row widths and alignment --------------------------------------------------------------------------------------------------------

def width_cases():
    """(words of P, c0, segments): the window ends near or at the end of the row"""
    return [(1, 15, LIST[:5]), (2, 30, LIST[:7]), (3, 37, LIST), (4, 60, LIST + [GOLAY, ID32]), (5, 37, LIST * 2),
            (64, 64 * 64 - 3 - 137 * 28, LIST * 28), (65, 129, LIST * 28), (65, 4000, LIST)]


def test_the_widths_reach_every_variant(dev):
    variants, lanes = set(), set()
    for nw, c0, segments in width_cases():
        ncols = 64 * nw - 3
        assert c0 + sum(c.n for c in segments) <= ncols
        plan = plan_of(dev, 300, ncols, segments)
        variants.add(plan[0])
        lanes.add(plan[4])
    probe = {plan_of(dev, 300, 8192, [ID32] * n)[0] for n in range(1, 257)}
    assert variants == probe == {0, 1} and lanes == {plan_of(dev, 300, 8192, [ID32] * n)[4] for n in range(1, 257)}
    assert [plan_of(dev, 300, 64 * nw - 3, s)[0] for nw, _, s in width_cases()] == [1, 1, 1, 1, 1, 0, 0, 1]


@pytest.mark.parametrize("layouts", LAYOUT_PAIRS, ids=lambda p: "P%d%d-D%d%d" % (p[0] + p[1]))
@pytest.mark.parametrize("case", width_cases(), ids=lambda c: "%dw-c%d" % c[:2])
def test_widths_and_alignment(dev, L, case, layouts):
    nw, c0, segments = case
    ncols = 64 * nw - 3
    N = R_of(dev) + 77                     # two passes
    words = g.random_words(N, ncols, nw + c0)
    run(dev, L, words, ncols, c0, segments, layouts=layouts)


# ---- row counts ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, "R-1", "R", "R+1", 70001])
@pytest.mark.parametrize("kind", ["staged", "global"])
def test_row_counts(dev, L, kind, n):
    R = R_of(dev)
    N = {"R-1": R - 1, "R": R, "R+1": R + 1}.get(n, n)
    ncols, c0, segments, variant = (128, 20, LIST[:6], 1) if kind == "staged" else (64 * 10, 7, LIST * 4, 0)
    words = g.random_words(N, ncols, 900 + N)
    run(dev, L, words, ncols, c0, segments, layouts=(OE, EE), variant=variant)


@pytest.mark.parametrize("kind", ["staged", "global"])
def test_more_passes_than_workgroups(dev, L, kind):
    """the workgroups loop: more rows than the most workgroups cover in one pass each"""
    R, G = R_of(dev), most_groups(dev)
    N = G * R + R + 5
    assert plan_of(dev, N, 128, [GOLAY])[8] == G and N < 1 << 21
    ncols, c0, segments, variant = (128, 41, [GOLAY, HAM3, ID32], 1) if kind == "staged" else (64 * 10, 3, [ID32] * 14 + [GOLAY, ID1], 0)
    words = g.random_words(N, ncols, N)
    run(dev, L, words, ncols, c0, segments, variant=variant)


# ---- streams, size ---------------------------------------------------------------------------------------------------------------------

def test_behind_pending_work_on_a_caller_stream(dev, L):
    """the pool is copied into its tensor on the caller's stream, behind a sleep; the reduction is enqueued twice behind it, into two
    destinations, before anything synchronises.  Both must hold what the reference makes of the pool, and the same bits."""
    import torch
    N, ncols, c0 = 20011, 256, 57
    segments = [GOLAY] * 6 + [HAM3, ID1]
    words = g.random_words(N, ncols, 0xC0DE)
    want_D, want_dist = cr.reduce(words, c0, segments)
    dsegs = [to_dev(dev, c) for c in segments]
    for code in dsegs:
        code.table_ptr()
    K = sum(c.k for c in segments)
    lane, = su.lanes([su.padded(words)])
    P = dev.DMat.from_torch(lane.live[0].reshape(N, -1), ncols)
    outs = []
    for _ in range(2):
        td = torch.full((N, 2), 0x1111111111111111, dtype=torch.int64, device="cuda")
        outs.append((td, dev.DMat.from_torch(td, K), guarded(N)))
    torch.cuda.synchronize()
    lane.open()
    for td, D, (tdist, pdist) in outs:
        dev.cover_reduce(P, c0, dsegs, D=D, dist=pdist, stream=lane.handle)
    pending = lane.pending()
    got = lane.read([td for td, _, _ in outs])
    torch.cuda.synchronize()
    assert pending, "the stream had drained before the calls were issued"
    for rows, (td, D, (tdist, pdist)) in zip(got, outs):
        assert np.array_equal(rows.reshape(N, 2), want_D) and np.array_equal(read_guarded(tdist), want_dist)


def test_a_view_of_a_parent_past_4gib(dev, L):
    """70 000 rows of 128 columns, 8192 words apart: the last rows start behind byte offset 2^32 of the parent.  Only the view's words
    are written (gf2_copy_block_dev from a compact upload); D is compact"""
    import torch
    N, ncols, ld, c0 = 70000, 128, 8192, 60
    segments = [GOLAY, HAM5, REP13]
    gc.collect()
    L.gf2_trim()
    torch.cuda.empty_cache()
    t = torch.empty((N, ld), dtype=torch.int64, device="cuda")
    assert N * ld * 8 > lr.LIMIT_BYTES
    words = g.random_words(N, ncols, 70)
    r_hi = lr.straddle(ld, N)[1]
    P = dev.DMat.wrap(t.data_ptr() + 8 * 6, N, ncols, ld, keep=t)
    dev.copy_block(P, 0, 0, dev.DMat.from_words(words, ncols), 0, 0, N, ncols)
    want_D, want_dist = cr.reduce(words, c0, segments)
    D, dist = dev.cover_reduce(P, c0, [to_dev(dev, c) for c in segments])
    got_D, got_dist = D.to_words(), dist.read(None)
    assert r_hi < N - 1 and np.array_equal(got_D, want_D) and np.array_equal(got_dist, want_dist)
    assert want_D[r_hi + 1:].any() and want_dist[r_hi + 1:].any()
    del t, P, D
    gc.collect()
    torch.cuda.empty_cache()


# ---- composition, end to end -----------------------------------------------------------------------------------------------------------

def reencoded(D, segments):
    """the codewords of the messages in D, side by side as the blocks were: words of sum(n) columns"""
    N = D.shape[0]
    bits = sum(c.n for c in segments)
    out = np.zeros((N, g.width(bits)), dtype=np.uint64)
    o = q = 0
    for code in segments:
        m = cr.blocks(D, q, code.k) if code.k else np.zeros(N, dtype=np.uint64)
        w = cr.encode(code, m)
        out[:, o >> 6] |= w << np.uint64(o & 63)
        if (o & 63) + code.n > 64:
            out[:, (o >> 6) + 1] |= w >> np.uint64(64 - (o & 63))
        o, q = o + code.n, q + code.k
    return out


def test_dist_is_the_distance_to_the_reencoded_rows(dev):
    """sum(dist) == count_ones(P's window XOR the codewords of D's messages): three device entries that agree through numpy"""
    N, ncols, c0 = 5000, 300, 41
    words = g.random_words(N, ncols, 41)
    P = dev.DMat.from_words(words, ncols)
    D, dist = dev.cover_reduce(P, c0, [to_dev(dev, c) for c in LIST])
    window = dev.submatrix(P, 0, c0, N, c0 + 137).to_words()
    away = window ^ reencoded(D.to_words(), LIST)
    got = dist.read(None)
    assert dev.count_ones(dev.DMat.from_words(away, 137)) == int(got.sum()) > 0
    assert np.array_equal(cr.popcount(away).sum(axis=1), got)
    assert np.array_equal(P.cover_reduce(c0, [to_dev(dev, c) for c in LIST]).to_words(), D.to_words())     # the method of the matrix


def lpn_pool(seed, extra=0, N=4096, tau=1 / 16):
    """N samples of 30 + extra bits at the columns [45 - extra, 75), the label at column 75.  The secret has weight 2 inside the 23
    bits of the Golay block and weight 1 inside the 7 bits behind it; its `extra` bits in front are random."""
    rng = np.random.default_rng(seed)
    secret = np.zeros(30 + extra, dtype=np.uint8)
    secret[:extra] = rng.integers(0, 2, extra)
    secret[extra + rng.choice(23, 2, replace=False)] = 1
    secret[extra + 23 + rng.integers(0, 7)] = 1
    samples = rng.integers(0, 2, (N, 30 + extra), dtype=np.uint8)
    errors = (rng.random(N) < tau).astype(np.uint8)
    label = (samples.astype(np.int64) @ secret.astype(np.int64) + errors) % 2
    bits = rng.integers(0, 2, (N, 100), dtype=np.uint8)              # the other columns are ignored
    bits[:, 45 - extra:75] = samples
    bits[:, 75] = label
    return g.bits_to_words(bits), secret[extra:]


def folded(secret):
    """the secret of the reduced pool: s_info ^ A^T s_par block by block (a codeword (u, A u) has <c, s> = <u, s_info ^ A^T s_par>)"""
    out, o, q = 0, 0, 0
    for code in (GOLAY, HAM3):
        s = sum(int(x) << j for j, x in enumerate(secret[o:o + code.n]))
        f = s & cr.mask(code.k)
        for t in range(code.n - code.k):
            if s >> (code.k + t) & 1:
                f ^= code.h[t] & cr.mask(code.k)
        out |= f << q
        o, q = o + code.n, q + code.k
    return out


def errors_reference(D, N):
    """the errors of all 2^16 secrets on the reduced pool: tally, transform, (N - F) / 2"""
    v = (D[:, 0] & np.uint64(0xFFFF)).astype(np.int64)
    sign = 1 - 2 * ((D[:, 0] >> np.uint64(16)) & np.uint64(1)).astype(np.int64)
    f = np.zeros(1 << 16, dtype=np.int64)
    np.add.at(f, v, sign)
    F = wr.as_int32(wr.wht_reference(f, 16)).astype(np.int64)
    assert not ((N - F) & 1).any()
    return ((N - F) // 2).astype(np.int32)


COVER = [GOLAY, HAM3, ID1]      # 31 bits from column 45 on, the label last: 17 columns, the label at column 16


@pytest.mark.parametrize("seed", [0, 7, 19])
def test_cover_end_to_end(dev, seed):
    """cover, the errors of all 2^16 secrets, the minimum -- one chain, one synchronisation at its end"""
    import torch
    words, secret = lpn_pool(seed)
    D_ref, _ = cr.reduce(words, 45, COVER)
    errors = errors_reference(D_ref, 4096)
    low = folded(secret)
    order = np.argsort(errors, kind="stable")
    assert order[0] == low and errors[order[0]] <= 1360 and errors[order[1]] >= 1898      # the reference alone recovers the secret
    dsegs = [to_dev(dev, c) for c in COVER]
    for code in dsegs:
        code.table_ptr()
    P = dev.DMat.from_words(words, 100)
    D = dev.DMat(4096, 17)
    te, pe = guarded(1 << 16)
    tm, pm = guarded(2)
    torch.cuda.synchronize()
    dev.cover_reduce(P, 45, dsegs, D=D, dist=dev.SKIP)
    dev.lpn_errors(D, 0, 16, 16, out=pe)
    dev.min_weight(pe, 1 << 16, idx=pm, val=pm + 4)
    torch.cuda.synchronize()
    assert np.array_equal(D.to_words(), D_ref)
    assert np.array_equal(read_guarded(te), errors)
    assert list(read_guarded(tm)) == [low, int(errors[low])]


@pytest.mark.parametrize("seed", [0, 7, 19])
def test_lf1_then_cover_end_to_end(dev, seed):
    """one LF1 round on four more sample bits in front, then the same chain"""
    import torch
    words, secret = lpn_pool(seed, extra=4)
    r1 = lf.lf1(words, 100, 41, 4)
    n1 = r1.D.shape[0]
    assert n1 == 4096 - 16
    D_ref, _ = cr.reduce(r1.D, 45, COVER)
    errors = errors_reference(D_ref, n1)
    low = folded(secret)
    order = np.argsort(errors, kind="stable")
    assert order[0] == low and errors[order[0]] < errors[order[1]]                         # the reference alone recovers the secret
    dsegs = [to_dev(dev, c) for c in COVER]
    for code in dsegs:
        code.table_ptr()
    P = dev.DMat.from_words(words, 100)
    D = dev.DMat(n1, 17)
    te, pe = guarded(1 << 16)
    tm, pm = guarded(2)
    torch.cuda.synchronize()
    D1, c1, _, _ = dev.lf1_reduce(P, 41, 4, cap=n1, src=dev.SKIP)
    dev.cover_reduce(D1, 45, dsegs, D=D, dist=dev.SKIP)
    dev.lpn_errors(D, 0, 16, 16, out=pe)
    dev.min_weight(pe, 1 << 16, idx=pm, val=pm + 4)
    torch.cuda.synchronize()
    assert int(c1.read(None)[0]) == n1
    assert np.array_equal(D.to_words(), D_ref)
    assert np.array_equal(read_guarded(te), errors)
    assert list(read_guarded(tm)) == [low, int(errors[low])]
