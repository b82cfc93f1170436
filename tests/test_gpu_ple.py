"""GPU tests of PLE / PLUQ (gf2_ple.hip): mzd_ple / mzd_pluq through the host entry (device path and size dispatch) and
gf2_ple_dev, bit for bit against the pure-Python model tests/ple_ref.py and the fixtures tests/golden/ple/*.npz; the
factorisation identity, Q against gf2_echelonize_dev and the row-rank-profile certificate at 16384^2; mzd_pluq_solve_left
against mzd_solve_left; gf2_apply_p_dev against the host functions."""
import ctypes
import glob
import os
import random

import numpy as np
import pytest

import gf2util as g
import ple_ref as R
from ple_cases import low_rank, structured

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    from m4ri_rust_amd import device
    device.require_gpu()
    return p


@pytest.fixture(params=["device", "dispatch"])
def mode(request, monkeypatch):
    if request.param == "dispatch":
        monkeypatch.delenv("M4RI_HIP_HOST_SMALL_WORK", raising=False)  # the library default
    else:
        monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", "0")
    return request.param


def host_ple(pkg, a, m, n, pluq):
    from m4ri_rust_amd import device
    L = pkg._lib.lib()
    M = pkg.BinMatrix.from_words(a, n)
    P, Q = device.Mzp(m), device.Mzp(n)
    r = (L.mzd_pluq if pluq else L.mzd_ple)(M.mzd, P.ptr, Q.ptr, 0)
    return r, P.to_list(), Q.to_list(), M.to_words()


def dev_ple(pkg, a, m, n, pluq):
    from m4ri_rust_amd import device
    A = device.DMat.from_words(a, n)
    r, P, Q = device.ple(A, pluq=pluq)
    return r, P, Q, A.to_words()


_EXPECT = {}


def expect(a, m, n, pluq):
    key = (a.tobytes(), m, n, pluq)
    if key not in _EXPECT:
        rank, P, Q, out = R.ple(R.rows_of(a, n), n, pluq)
        _EXPECT[key] = rank, P, Q, R.words_of_rows(out, n)
    return _EXPECT[key]


def same(got, want):
    assert got[0] == want[0], ("rank", got[0], want[0])
    assert got[1] == want[1], "P differs"
    assert got[2] == want[2], "Q differs"
    assert np.array_equal(got[3], want[3]), "in-place result differs"


SHAPES = [(1, 1), (63, 65), (64, 64), (65, 129), (200, 1000), (1000, 200), (1000, 1000)]


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("pluq", [False, True])
def test_host_entry_random(pkg, mode, m, n, pluq):
    a = g.random_words(m, n, m + 3 * n)
    same(host_ple(pkg, a, m, n, pluq), expect(a, m, n, pluq))


@pytest.mark.parametrize("m,n", SHAPES)
def test_dev_random_and_low_rank(pkg, m, n):
    for r in (0, 1, 63, 64, 65, 700):
        if r > min(m, n):
            continue
        a = low_rank(m, n, r, r + m)
        for pluq in (False, True):
            same(dev_ple(pkg, a, m, n, pluq), expect(a, m, n, pluq))


@pytest.mark.parametrize("m,n", [(63, 65), (200, 1000), (1000, 200)])
@pytest.mark.parametrize("pluq", [False, True])
def test_structured(pkg, mode, m, n, pluq):
    for a in structured(m, n):
        same(host_ple(pkg, a, m, n, pluq), expect(a, m, n, pluq))
        same(dev_ple(pkg, a, m, n, pluq), expect(a, m, n, pluq))


def test_golden_fixtures_on_device(pkg, monkeypatch):
    monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", "0")
    files = sorted(glob.glob(os.path.join(HERE, "golden", "ple", "*.npz")))
    assert files
    for f in files:
        z = np.load(f)
        m, n = int(z["m"]), int(z["n"])
        for pluq, key in ((False, "ple"), (True, "pluq")):
            for got in (host_ple(pkg, z["a"], m, n, pluq), dev_ple(pkg, z["a"], m, n, pluq)):
                same(got, (int(z["rank"]), z["P"].tolist(), z["Q"].tolist(), z[key]))


def test_dirty_window(pkg, monkeypatch):
    from m4ri_rust_amd import device
    monkeypatch.setenv("M4RI_HIP_HOST_SMALL_WORK", "0")
    L = pkg._lib.lib()
    m, n, r0, c0 = 300, 700, 5, 64
    pc = c0 + n + 70
    for pluq in (False, True):
        parent = pkg.BinMatrix.from_words(g.random_words(r0 + m + 3, pc, 77), pc)
        w = g.width(pc)
        parent._words_view()[:, :w] = g.splitmix64(99 + pluq, np.arange((r0 + m + 3) * w, dtype=np.uint64)).reshape(-1, w)
        before = g.words_to_bits(parent.to_words(), w * 64)
        a = g.bits_to_words(before[r0:r0 + m, c0:c0 + n].copy())
        W = L.mzd_init_window(parent.mzd, r0, c0, r0 + m, c0 + n)
        P, Q = device.Mzp(m), device.Mzp(n)
        rank = (L.mzd_pluq if pluq else L.mzd_ple)(W, P.ptr, Q.ptr, 0)
        L.mzd_free(W)
        after = g.words_to_bits(parent.to_words(), w * 64)
        mask = np.ones_like(after, dtype=bool)
        mask[r0:r0 + m, c0:c0 + n] = False
        assert np.array_equal(after[mask], before[mask]), "parent changed outside the window"
        same((rank, P.to_list(), Q.to_list(), g.bits_to_words(after[r0:r0 + m, c0:c0 + n].copy())), expect(a, m, n, pluq))


def test_2049x3000_identity(pkg):
    m, n = 2049, 3000
    a = low_rank(m, n, 1500, 5)
    check_large(pkg, a, m, n, certificate=True)


def split_words(out, rank, n):
    """in-place result (m x w words) -> (L: m x rank with unit diagonal, E/U: rank x n)"""
    m = out.shape[0]
    i = np.arange(m, dtype=np.int64)[:, None]
    def lowmask(lim, words):
        bits = np.clip(lim - 64 * np.arange(words, dtype=np.int64)[None, :], 0, 64)
        with np.errstate(over="ignore"):
            return np.where(bits >= 64, np.uint64(0xFFFFFFFFFFFFFFFF),
                            (np.uint64(1) << np.minimum(bits, 63).astype(np.uint64)) - np.uint64(1)).astype(np.uint64)
    lw = g.width(max(rank, 1))
    Lw = np.ascontiguousarray(out[:, :lw] & lowmask(np.minimum(i, rank), lw))
    diag = np.arange(min(rank, m))
    Lw[diag, diag // 64] |= np.uint64(1) << (diag % 64).astype(np.uint64)
    if rank % 64:
        Lw[:, -1] &= np.uint64((1 << (rank % 64)) - 1)
    Ew = np.ascontiguousarray(out[:rank] & ~lowmask(i[:rank], out.shape[1]))
    return Lw, Ew


def check_large(pkg, a, m, n, certificate):
    from m4ri_rust_amd import device
    for pluq in (False, True):
        A = device.DMat.from_words(a, n)
        rank, P, Q = device.ple(A, pluq=pluq)
        out = A.to_words()
        # two runs give identical output
        A2 = device.DMat.from_words(a, n)
        assert device.ple(A2, pluq=pluq) == (rank, P, Q) and device.equal(A, A2)
        Lw, Ew = split_words(out, rank, n)
        lhs = device.DMat.from_words(a, n)
        device.apply_p(lhs, P)
        if pluq:
            device.apply_p(lhs, Q, right=True, trans=True)
        if rank:
            prod = device.mul(device.DMat.from_words(Lw, rank), device.DMat.from_words(Ew, n))
            assert device.equal(prod, lhs), "P A0 (Q^T) != L E (L U)"
        else:
            assert not lhs.to_words().any()
        if not pluq:
            er, piv = device.echelonize(device.DMat.from_words(a, n), full=False)
            assert er == rank and Q[:rank] == piv
            # echelon structure: the lowest set bit of E_k is Q[k]
            bits = g.words_to_bits(Ew, n) if rank else np.zeros((0, n), np.uint8)
            assert all(int(np.argmax(bits[k])) == Q[k] for k in range(rank))
            if certificate:
                # with P A0 = L E above and E of full row rank, this makes the pivot rows the row rank profile
                sigma = R.apply_left(list(range(m)), P)
                lb = g.words_to_bits(Lw, max(rank, 1))[:, :rank]
                piv_rows = np.array(sigma[:rank])
                for i in range(rank, m):
                    ks = np.nonzero(lb[i])[0]
                    assert (piv_rows[ks] < sigma[i]).all(), "a non-pivot row depends on a later pivot row"
        check_orders(P, Q, rank, m)


def check_orders(P, Q, rank, m):
    """P is a permutation whose non-pivot rows keep their input order; Q[:rank] (the pivot columns) strictly increases."""
    sigma = np.array(R.apply_left(list(range(m)), P))
    assert np.array_equal(np.sort(sigma), np.arange(m)), "P does not realise a permutation"
    assert (np.diff(sigma[rank:]) > 0).all(), "the non-pivot rows are not in their original order"
    assert (np.diff(np.asarray(Q[:rank])) > 0).all(), "the pivot columns do not increase"


@pytest.mark.parametrize("kind", ["random", "rank10000"])
def test_16384(pkg, kind):
    n = 16384
    a = g.random_words(n, n, 3) if kind == "random" else low_rank(n, n, 10000, 8)
    check_large(pkg, a, n, n, certificate=True)


def _lowmask_t(torch, lim, words):
    """(rows, words) int64 masks of the bits below column lim[i] (lim: int64 tensor of shape (rows,))"""
    bits = (lim[:, None] - 64 * torch.arange(words, device=lim.device, dtype=torch.int64)[None, :]).clamp(0, 64)
    one = torch.ones((), dtype=torch.int64, device=lim.device)
    m = torch.bitwise_left_shift(one, bits.clamp(max=63)) - 1
    return torch.where(bits >= 64, torch.full_like(m, -1), m)


def check_on_device(pkg, src, n, want_rank):
    """PLE and PLUQ of the n x n device matrix `src`, checked on the device: P A0 (Q^T) == L E (L U) through gf2_mul_dev and
    gf2_equal_dev; r and Q[:r] against gf2_echelonize_dev; the in-place layout (zeros between the diagonal and Q[i], E_i leading at
    Q[i], U_i at the diagonal, nothing right of column r in the rows below r); a second run equal to the first."""
    import torch
    from m4ri_rust_amd import device
    w = g.width(n)
    ld = w + (w & 1)

    def copy_of_src():
        t = torch.zeros((n, ld), dtype=torch.int64, device="cuda")
        D = device.DMat.from_torch(t, n)
        device.add(src, device.add(src, src), C=D)  # D = src ^ 0
        return t, D

    er, piv = device.echelonize(copy_of_src()[1], full=False)
    assert er == want_rank
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    for pluq in (False, True):
        t, A = copy_of_src()
        rank, P, Q = device.ple(A, pluq=pluq)
        assert rank == er and Q[:rank] == piv and Q[rank:] == list(range(rank, n))
        check_orders(P, Q, rank, n)
        t2, A2 = copy_of_src()
        assert device.ple(A2, pluq=pluq) == (rank, P, Q) and device.equal(A, A2), "two runs differ"
        del t2, A2
        out = t[:, :w]
        q = torch.tensor(Q, device="cuda", dtype=torch.int64)
        low_i = _lowmask_t(torch, i[:rank], w)
        top = out[:rank]
        if not pluq:
            assert not (top & _lowmask_t(torch, q[:rank], w) & ~low_i).any(), "bits between the diagonal and Q[i]"
        qi = i[:rank] if pluq else q[:rank]
        lead = torch.gather(top, 1, (qi // 64)[:, None])[:, 0]
        assert bool(((torch.bitwise_right_shift(lead, qi % 64) & 1) == 1).all()), "E_i / U_i does not lead where it should"
        if rank < n:
            lim = torch.full((n - rank,), rank, device="cuda", dtype=torch.int64)
            assert not (out[rank:] & ~_lowmask_t(torch, lim, w)).any(), "bits right of column r in a row below r"
        # L (n x r, unit diagonal) and E / U (r x n), split on the device
        lw = g.width(rank)
        Lt = torch.zeros((n, lw + (lw & 1)), dtype=torch.int64, device="cuda")
        Lt[:, :lw] = out[:, :lw] & _lowmask_t(torch, torch.clamp(i, max=rank), lw)
        d = i[:rank]
        Lt[d, d // 64] |= torch.bitwise_left_shift(torch.ones_like(d), d % 64)
        Et = torch.zeros((rank, ld), dtype=torch.int64, device="cuda")
        Et[:, :w] = top & ~low_i
        prod = device.mul(device.DMat.from_torch(Lt, rank), device.DMat.from_torch(Et, n))
        lt, lhs = copy_of_src()
        device.apply_p(lhs, P)
        if pluq:
            device.apply_p(lhs, Q, right=True, trans=True)
        assert device.equal(prod, lhs), "P A0 (Q^T) != L E (L U)"
        del t, A, Lt, Et, prod, lt, lhs
        torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["random", "rank40000"])
def test_65536_on_device(pkg, kind):
    from m4ri_rust_amd import device
    n = 65536
    if kind == "random":
        src = device.DMat.random(n, n, 21)
        want = device.echelonize(src.clone(), full=False)[0]
    else:
        src = device.mul(device.DMat.random(n, 40000, 22), device.DMat.random(40000, n, 23))
        want = 40000
    check_on_device(pkg, src, n, want)


def launches(L):
    need = L.gf2_kernel_census(None, 0)
    buf = ctypes.create_string_buffer(need + 1)
    L.gf2_kernel_census(buf, need + 1)
    out = {}
    for ln in buf.value.decode().splitlines():
        parts = ln.split(None, 1)
        if len(parts) == 2 and parts[0].isdigit():
            out[parts[1].strip()] = out.get(parts[1].strip(), 0) + int(parts[0])
    return out


def test_large_host_column_permutation_takes_the_device(pkg):
    """mzd_apply_p_right* of >= 2^24 bits runs on the device: the numpy column gather's bits, the parent of a window intact"""
    from m4ri_rust_amd import device
    L = pkg._lib.lib()
    m, n = 1500, 12000
    rng = random.Random(5)
    perm = [rng.randrange(i, n) for i in range(n)]
    hp = device.Mzp.from_list(perm)
    for trans in (False, True):
        at = list(range(n))
        for i in (range(n) if trans else reversed(range(n))):
            at[i], at[perm[i]] = at[perm[i]], at[i]
        for window in (False, True):
            pc = 64 + n + 70 if window else n
            parent = pkg.BinMatrix.from_words(g.random_words(m + 4, pc, 31), pc)
            wds = g.width(pc)
            parent._words_view()[:, :wds] = g.splitmix64(32 + trans, np.arange((m + 4) * wds, dtype=np.uint64)).reshape(-1, wds)
            before = g.words_to_bits(parent.to_words(), wds * 64)
            r0, c0 = (2, 64) if window else (0, 0)
            W = L.mzd_init_window(parent.mzd, r0, c0, r0 + m, c0 + n)
            k0 = launches(L)
            (L.mzd_apply_p_right_trans if trans else L.mzd_apply_p_right)(W, hp.ptr)
            k1 = launches(L)
            L.mzd_free(W)
            after = g.words_to_bits(parent.to_words(), wds * 64)
            want = before.copy()
            want[r0:r0 + m, c0:c0 + n] = before[r0:r0 + m, c0:c0 + n][:, at]
            assert np.array_equal(after, want)
            assert any("ple_gather" in k and k1[k] > k0.get(k, 0) for k in k1), "the device route did not run"


def solve_case(pkg, m, n, k, r, consistent, check, seed):
    L = pkg._lib.lib()
    from m4ri_rust_amd import device
    a = low_rank(m, n, r, seed)
    b = g.o_mul_naive(a, g.random_words(n, k, seed + 2), m, n, k) if consistent else g.random_words(m, k, seed + 3)
    brows = max(m, n)
    bfull = np.vstack([b, g.random_words(brows - m, k, seed + 4)]) if brows > m else b
    # reference: mzd_solve_left on a copy of A0
    A1, B1 = pkg.BinMatrix.from_words(a, n), pkg.BinMatrix.from_words(bfull, k)
    rc1 = L.mzd_solve_left(A1.mzd, B1.mzd, 0, check)
    A2, B2 = pkg.BinMatrix.from_words(a, n), pkg.BinMatrix.from_words(bfull, k)
    P, Q = device.Mzp(m), device.Mzp(n)
    rank = L.mzd_pluq(A2.mzd, P.ptr, Q.ptr, 0)
    rc2 = L.mzd_pluq_solve_left(A2.mzd, rank, P.ptr, Q.ptr, B2.mzd, 0, check)
    assert rc2 == rc1
    if consistent:
        assert rc2 == 0
        assert np.array_equal(B2.to_words(), B1.to_words())
        assert np.array_equal(g.o_mul_naive(a, B2.to_words()[:n], m, n, k), b)
    return rc2


@pytest.mark.parametrize("m,n", [(500, 500), (300, 700), (700, 300)])
@pytest.mark.parametrize("k", [1, 64, 300])
def test_pluq_solve_left(pkg, mode, m, n, k):
    r = min(m, n) - 37
    for check in (0, 1):
        solve_case(pkg, m, n, k, r, True, check, m + n + k)
    assert solve_case(pkg, m, n, k, r, False, 1, 3 * k) == -1


def test_pluq_solve_left_device_api(pkg):
    from m4ri_rust_amd import device
    m, n, k = 900, 900, 70
    a = low_rank(m, n, 800, 4)
    b = g.o_mul_naive(a, g.random_words(n, k, 5), m, n, k)
    A = device.DMat.from_words(a, n)
    rank, P, Q = device.ple(A, pluq=True)
    B = device.DMat.from_words(b, k)
    assert device.pluq_solve_left(A, rank, P, Q, B, check=True)
    x = B.to_words()
    assert np.array_equal(g.o_mul_naive(a, x, m, n, k), b)
    bad = device.DMat.from_words(g.random_words(m, k, 6), k)
    assert not device.pluq_solve_left(A, rank, P, Q, bad, check=True)


@pytest.mark.parametrize("m,n", [(70, 130), (1000, 3000), (3000, 1000)])
def test_apply_p_dev_matches_host(pkg, m, n):
    from m4ri_rust_amd import device
    L = pkg._lib.lib()
    rng = random.Random(m * n)
    a = g.random_words(m, n, 17)
    for right in (False, True):
        size = n if right else m
        perm = [rng.randrange(i, size) for i in range(size)]
        for trans in (False, True):
            D = device.DMat.from_words(a, n)
            device.apply_p(D, perm, right=right, trans=trans)
            H = pkg.BinMatrix.from_words(a, n)
            fn = "mzd_apply_p_" + ("right" if right else "left") + ("_trans" if trans else "")
            hp = device.Mzp.from_list(perm)
            getattr(L, fn)(H.mzd, hp.ptr)
            assert np.array_equal(D.to_words(), H.to_words()), fn
