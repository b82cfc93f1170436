"""gf2_mul_dev, gf2_mul_nt_dev and gf2_transpose_dev on 8-byte-aligned views of dirty parents (include/m4ri_hip.h section 2: "accepts
8-byte-aligned rows"): every operand is a window of a caller's buffer (tests/dev_views.py) with an odd or even `ld` and a first word
that is or is not 16-byte aligned, or a column range of a wider matrix (WIDE), and every word of the parent outside the window holds
random bits.  Almost every kernel behind these entries picks a 16-byte or an 8-byte form per operand from the address it is given;
each of those branches can read or write one word too far or skip the mask of the last word, which shows only when the words around
the view are not zero.  The host (mzd_t) entries of tests/test_gpu_views.py upload into fresh, naturally strided blocks: their
kernels never see a caller's stride.

Every case asserts, after one synchronisation, bit for bit against the CPU oracle (never against another device result):
  1. the window of C (D) is the oracle's product (xor the initial C when accumulating), all rows;
  2. the excess bits of its last word are zero;
  3. every other word of its parent is as uploaded -- the rows above and below, the words left and right, the words up to `ld`;
  4. the parents of A and B (Bt, S) are unchanged;
  5. the kernel family the case is meant for launched (launch census).  The shapes were picked with the planner's queries, which
     need no device, and each case asserts the plan first, so that a moved threshold fails the case instead of re-routing it.

Routes that no shape reaches through gf2_mul_dev (plain_path, mul_naive_dev and widevec_shape / ts_long_shape of mul_plan_host.cpp)
and that are therefore absent from ROUTES:
  - the wave-per-row kernel in two passes (33-64 vectors): it asks for l >= 16384 (or m <= 8 and l >= 8192), and from 17 vectors and
    l >= 2048 on the slab-table kernel is asked first and takes the shape.  The second pass is reached through gf2_mul_nt_dev, which
    asks widevec_shape alone (NT_WIDEVEC below);
  - the two-kernel naive path (gf2_transpose + gf2_rowparity_kernel) of mul_naive_dev: it needs n * ceil(l / 64) * 8 > 65536 with
    n <= 64, that is l > 8192; from l >= 2048 on the wave-per-row kernel (n <= 16) or the slab tables (n > 16) take the shape first.

The GPU cases carry the `gpu` mark one by one, not through `pytestmark`: the cases at the top check tests/dev_views.py's own claims on
CPU tensors and belong to the suite that runs without a device."""
import ctypes
import functools

import numpy as np
import pytest

import dev_views as dv
import gf2util as g
from census_util import assert_route, census
from dev_views import EE, EO, OE, OO, WIDE, View

gpu = pytest.mark.gpu

# (A, B, C): every operand takes each of EE, EO, OE, OO at least once and is at least once the only one that is not EE
TRIPLES = [(EE, EE, EE), (OO, EE, EE), (EE, OO, EE), (EE, EE, OO), (EO, OE, OO), (OE, EO, EO), (OO, OO, OE), (WIDE, WIDE, WIDE)]
TRIPLE_IDS = ["-".join(t) for t in TRIPLES]
# (S, D) of the transposition
PAIRS = [(EE, EE), (OO, EE), (EE, OO), (EO, OE), (OE, EO), (OO, OO), (WIDE, WIDE)]
PAIR_IDS = ["-".join(p) for p in PAIRS]


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


# ---- the helper's own claims (no GPU) ---------------------------------------------------------------------------------------------

def test_the_triples_cover_every_layout():
    for k in range(3):
        assert {t[k] for t in TRIPLES} >= {EE, EO, OE, OO, WIDE}
        assert any(t[k] not in (EE, WIDE) and all(t[j] == EE for j in range(3) if j != k) for t in TRIPLES)


@pytest.mark.parametrize("layout", dv.LAYOUTS)
@pytest.mark.parametrize("nrows,ncols", [(5, 1), (3, 64), (7, 65), (4, 200), (2, 257)])
def test_view_layouts(layout, nrows, ncols):
    """View on a CPU tensor: parity of `ld`, parity of the first word, the window's content, the rows and words around it, and
    expect() differing from the parent in the window's words only"""
    words = g.random_words(nrows, ncols, 7 + ncols)
    V = View(None, nrows, ncols, layout, 1000 + nrows, words)
    w = g.width(ncols)
    ld_odd, base_odd = {EE: (0, 0), EO: (0, 1), OE: (1, 0), OO: (1, 1), WIDE: (0, 0)}[layout]
    assert V.m is None and V.t.data_ptr() % 16 == 0
    assert V.ld & 1 == ld_odd and ((V.base - V.t.data_ptr()) // 8) & 1 == base_odd and (V.base // 8) & 1 == base_odd
    if layout == WIDE:
        assert V.ld >= 2 * w and V.base % 16 == 0
    parent = V.read()
    assert parent.shape == (nrows + 3, V.ld) and dv.R0 >= 1 and dv.BELOW >= 2 and V.cw >= 1 and V.ld - V.cw - w >= 1
    assert np.array_equal(V.window(parent), words) and np.array_equal(V.window(), words)
    first = (V.base - V.t.data_ptr()) // 8   # the window starts where the gf2_dmat would point
    assert np.array_equal(parent.reshape(-1)[first:first + w], words[0])
    outside = np.ones(parent.shape, dtype=bool)
    outside[dv.R0:dv.R0 + nrows, V.cw:V.cw + w] = False
    assert (parent[outside] != 0).mean() > 0.9, "the words around the window are not dirty"
    # another seed, the same window: only the surroundings differ
    other = View(None, nrows, ncols, layout, 2000 + nrows, words).read()
    assert np.array_equal(V.window(other), words) and (other[outside] != parent[outside]).mean() > 0.9
    V.unchanged()
    rows = ~words
    want = V.expect(rows)
    assert np.array_equal(want[outside], parent[outside]) and np.array_equal(V.window(want), rows) and (want != parent).sum() == nrows * w
    V.t[0, 0] ^= 1
    with pytest.raises(AssertionError):
        V.unchanged()


def test_view_refuses_dirty_excess_bits():
    words = g.random_words(3, 70, 1)
    words[1, -1] |= np.uint64(1 << 6)
    with pytest.raises(AssertionError):
        View(None, 3, 70, EE, 1, words)


# ---- planner queries (no device) --------------------------------------------------------------------------------------------------

def tile_plan(dev, m, l, n, batch=1, packed=0):
    out = (ctypes.c_longlong * 9)()
    dev._lib.lib().gf2_tile_plan(m, l, n, batch, packed, out)
    return list(out)


def mul_plan(dev, m, l, n, algo, param):
    kind, dims = ctypes.c_int(0), (ctypes.c_int * 3)()
    levels = dev._lib.lib().gf2_mul_plan(m, l, n, dev.ALGOS[algo], param, ctypes.byref(kind), dims)
    return levels, kind.value, list(dims)


def ws_bytes(dev, m, l, n, algo, param=0):
    return dev._lib.lib().gf2_mul_workspace_bytes(m, l, n, dev.ALGOS[algo], param)


def even(w):
    return (w + 1) & ~1


def packed_bytes(m, l):
    return ((m + 63) & ~63) * even(g.width(l)) * 8


def plan_by_census(dev, m, l, n, algo):   # mul_naive_dev's own thresholds: no query tells these kernels apart, the census does
    assert n <= 8 and ws_bytes(dev, m, l, n, algo) == n * even(g.width(l)) * 8, ("the planner runs this shape another way: pick another shape", (m, l, n))


def plan_whole_rounds(dev, m, l, n, algo):
    p = tile_plan(dev, m, l, n)
    assert p[0] in (9, 10, 11, 12) and p[2] == 0 and p[4] == 0, ("no longer whole v8 tiles: pick another shape", (m, l, n), p)


def plan_streamk(dev, m, l, n, algo):
    p = tile_plan(dev, m, l, n)
    assert p[0] in (9, 10, 11, 12) and p[2] > 0 and p[4] > 0, ("no stream-K cut any more: pick another shape", (m, l, n), p)
    assert ws_bytes(dev, m, l, n, algo) == p[4], ("A is packed now: pick another shape", (m, l, n), p)


def plan_splitk(variants):
    def check(dev, m, l, n, algo):
        p = tile_plan(dev, m, l, n)
        assert p[0] in variants and p[1] > 1 and p[4] > 0, ("no longer split-K with variant %s: pick another shape" % (variants,), (m, l, n), p)
        assert ws_bytes(dev, m, l, n, algo) == p[4], ("A is packed now: pick another shape", (m, l, n), p)
    return check


def plan_packed(dev, m, l, n, algo):
    p = tile_plan(dev, m, l, n, 1, 1)
    assert p[4] > 0 and ws_bytes(dev, m, l, n, algo) == p[4] + packed_bytes(m, l), ("A is no longer packed: pick another shape", (m, l, n), p)


def plan_no_scratch(dev, m, l, n, algo):   # the table, slab, narrow and v*A kernels work in place
    assert ws_bytes(dev, m, l, n, algo) == 0, ("the planner runs this shape another way: pick another shape", (m, l, n))


def plan_transposed_vectors(dev, m, l, n, algo):   # the wave-per-row kernel: B transposed into scratch
    assert ws_bytes(dev, m, l, n, algo) == n * even(g.width(l)) * 8, ("no longer the wave-per-row path: pick another shape", (m, l, n))


def plan_few_rows_t(dev, m, l, n, algo):   # computed transposed: B^T, A^T, C^T and a copy of the product when accumulating
    want = (n * even(g.width(l)) + 2 * l + n * even(g.width(m)) + m * even(g.width(n))) * 8
    assert 8 < m <= 128 and ws_bytes(dev, m, l, n, algo) == want, ("no longer the transposed few-rows path: pick another shape", (m, l, n))


def plan_strassen(levels, kind, dims=None):
    def check(dev, m, l, n, algo):
        got = mul_plan(dev, m, l, n, "strassen", levels)
        assert got[:2] == (levels, kind), ("the planner runs this shape another way: pick another shape", (m, l, n), got)
        if dims is not None:
            assert got[2] == list(dims), ("another padded shape or core: pick another shape", (m, l, n), got)
    return check


# ---- products, computed once per shape and never written --------------------------------------------------------------------------

def _oracle_mul(a, b, m, l, n):
    return (g.o_mul_fast if max(m, l, n) >= 4096 else g.o_mul_m4rm)(a, b, m, l, n)   # as tests/test_gpu_views.py chooses


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def product(m, l, n, seed):
    """(a, b, c0, a * b)"""
    a, b, c0 = g.random_words(m, l, seed), g.random_words(l, n, seed + 1), g.random_words(m, n, seed + 2)
    return _frozen(a, b, c0, _oracle_mul(a, b, m, l, n))


@functools.lru_cache(maxsize=None)
def product_nt(m, l, n, seed):
    """(a, bt, c0, a * bt^T), bt as n x l"""
    a, bt, c0 = g.random_words(m, l, seed), g.random_words(n, l, seed + 1), g.random_words(m, n, seed + 2)
    return _frozen(a, bt, c0, _oracle_mul(a, g.o_transpose(bt, n, l), m, l, n))


@functools.lru_cache(maxsize=None)
def transposed(m, n, seed):
    s = g.random_words(m, n, seed)
    return _frozen(s, g.o_transpose(s, m, n))


def launched(before, after):
    return sorted(k for k, v in after.items() if v > before.get(k, 0))


def check_c(C, want, what):
    """1-3 of the module's list for the destination view C"""
    got = C.read()
    win = C.window(got)
    if C.ncols % 64:
        assert not (win[:, -1] >> np.uint64(C.ncols % 64)).any(), (what, "excess bits of the last word are not zero")
    bad = np.argwhere(win != want)
    assert not len(bad), (what, "%d wrong words in the window, first at (row, word) %s" % (len(bad), tuple(bad[0])))
    exp = C.expect(want)
    bad = np.argwhere(got != exp)
    assert not len(bad), (what, "%d words of the parent outside the window changed, first at parent (row, word) %s; the window is rows "
                          "%d.., words %d..%d of %d" % (len(bad), tuple(bad[0]), dv.R0, C.cw, C.cw + C.w - 1, C.ld))


def run_products(dev, L, call, ops, cols, layouts, families, what, seed=0):
    """call(A, B, C, accumulate) on views of ops = (a, b, c0, product), plain and accumulating; b is whatever the entry takes second
    (B or Bt), cols = the columns of (a, b, c0).  -> the kernels launched by the plain and by the accumulating call"""
    import torch
    a, b, c0, prod = ops
    m, n = a.shape[0], cols[2]
    A = View(dev, m, cols[0], layouts[0], 3 * seed + 1, a)
    B = View(dev, b.shape[0], cols[1], layouts[1], 3 * seed + 2, b)
    ran = []
    for acc in (False, True):
        C = View(dev, m, n, layouts[2], 3 * seed + 3 + acc, c0)   # plain: C's old content must be overwritten, not merged
        torch.cuda.synchronize()
        k0 = census(L)
        call(A.m, B.m, C.m, acc)
        torch.cuda.synchronize()
        k1 = census(L)
        tag = (what, layouts, "accumulate" if acc else "plain")
        check_c(C, prod ^ c0 if acc else prod, tag)
        A.unchanged("A %s" % (tag,))
        B.unchanged("B %s" % (tag,))
        if families is not None:
            assert_route(k0, k1, families)
        ran.append(launched(k0, k1))
    return ran


# ---- gf2_mul_dev: the plain routes ------------------------------------------------------------------------------------------------

# (route, algo, m, l, n, kernel families that must launch -- a function of the layouts where the launcher picks the instantiation by
# A's alignment --, plan check).  The first twelve are tests/test_gpu_views.py's ROUTES, the
# smallest shapes known to reach each route; the others were found with the planner queries: the smallest of a grid of shapes
# one above a power of two
ROUTES = [
    ("v8-whole-rounds", "m4rm", 257, 65, 65, ["gf2_m4rm_kernel_v8"], plan_whole_rounds),
    ("v8-streamk", "m4rm", 1000, 1025, 4097, ["gf2_m4rm_kernel_v8", "gf2_streamk_reduce_kernel"], plan_streamk),
    ("v3-splitk", "m4rm", 100, 5001, 97, ["gf2_m4rm_kernel_v3", "gf2_splitk_reduce_kernel"], plan_splitk((7, 20))),
    ("v6-splitk", "m4rm", 6001, 4097, 4097, ["gf2_m4rm_kernel_v6", "gf2_splitk_reduce_kernel"], plan_splitk((8,))),
    # (six words of A per row: 16-byte loads into gf2_narrow_kernel<8> when A allows them, the loop form <0> otherwise)
    ("narrow", "naive", 5001, 321, 1, lambda lay: ["gf2_narrow_kernelILi%dEE" % (8 if lay[0] in (EE, WIDE) else 0)], plan_by_census),
    ("lpnvec", "naive", 262401, 255, 1, ["gf2_lpnvec_kernel"], plan_by_census),
    ("lpn8", "m4rm", 20001, 255, 32, ["gf2_lpn8_kernel"], plan_no_scratch),
    ("lpn256", "m4rm", 20001, 193, 160, ["gf2_lpn256_kernel"], plan_no_scratch),
    ("tallskinny3", "m4rm", 524289, 321, 96, ["gf2_tallskinny3_kernel"], plan_no_scratch),
    ("tallskinny7", "naive", 65601, 705, 1, ["gf2_tallskinny7_kernel"], plan_no_scratch),
    ("tallskinny7-wide", "m4rm", 3001, 2113, 32, ["gf2_tallskinny7_kernel"], plan_no_scratch),
    ("widevec", "naive", 3001, 1025, 1, ["gf2_widevec_kernel"], plan_transposed_vectors),
    # A packed by a pass of its own in front of a stream-K launch
    ("packed-a", "m4rm", 513, 8193, 1025, ["gf2_packA_kernel", "gf2_m4rm_kernel_v8", "gf2_streamk_reduce_kernel"], plan_packed),
    # m <= 8: B streamed once
    ("va", "m4rm", 3, 1025, 2017, ["gf2_va_kernel"], plan_no_scratch),
    # 9-128 rows against a tall B, computed transposed; 70 rows: two passes of 64, the second from A->data + 64 * A->ld
    ("few-rows-transposed", "m4rm", 70, 16385, 131, ["gf2_transpose_kernel", "gf2_tallskinny7_kernel"], plan_few_rows_t),
    # 65-128 columns through the slab tables with two words per row of C (kPathSlabPasses, one pass) ...
    ("slab-128", "m4rm", 301, 2049, 100, ["gf2_tallskinny7_kernelILi4ELi2E"], plan_no_scratch),
    # ... and 193-256 columns in two passes, the second at B->data + 2 and C->data + 2
    ("slab-two-passes", "m4rm", 4097, 32769, 200, ["gf2_tallskinny7_kernelILi4ELi2E"], plan_no_scratch),
    # the wave-per-row kernel with 9-16 vectors (the two-pass form: the module's docstring)
    ("widevec-16", "m4rm", 300, 2049, 13, ["gf2_widevec_kernelILi16E"], plan_transposed_vectors),
]


@gpu
@pytest.mark.parametrize("layouts", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("route,algo,m,l,n,families,plan", ROUTES, ids=[r[0] for r in ROUTES])
def test_mul_dev_routes_on_views(dev, L, route, algo, m, l, n, families, plan, layouts):
    plan(dev, m, l, n, algo)
    seed = 100 + 10 * [r[0] for r in ROUTES].index(route)
    call = lambda A, B, C, acc: dev.mul(A, B, C, accumulate=acc, algo=algo)  # noqa: E731
    fams = families(layouts) if callable(families) else families
    run_products(dev, L, call, product(m, l, n, seed), (l, n, n), layouts, fams, (route, m, l, n), seed)


# ---- gf2_mul_dev: Strassen --------------------------------------------------------------------------------------------------------

# (name, levels asked for, m, l, n, families under EE and WIDE, plan check).  Forced levels at the smallest shapes the level plan
# divides; the padded plan; the peeled plans: the smallest shape for which gf2_mul_plan gives kind 2 (it peels the tail of the
# inner dimension only) and the smallest of the same grid with all three border strips
STRASSEN = [
    ("levels-1", 1, 128, 256, 256, ["gf2_strassen_"], plan_strassen(1, 0)),
    ("levels-2", 2, 256, 512, 512, ["gf2_strassen_"], plan_strassen(2, 0)),
    ("levels-3", 3, 512, 1024, 1024, ["gf2_strassen_"], plan_strassen(3, 0)),
    ("levels-4", 4, 16, 2048, 2048, ["gf2_strassen_"], plan_strassen(4, 0)),
    ("padded", 2, 2113, 2144, 2175, ["gf2_padcopy_kernel", "gf2_strassen_"], plan_strassen(2, 1, (2304, 2560, 2560))),
    ("peeled-inner", 3, 1024, 2049, 2048, ["gf2_strassen_"], plan_strassen(3, 2, (1024, 2048, 2048))),
    ("peeled-three-strips", 4, 1025, 2113, 8257, ["gf2_strassen_"], plan_strassen(4, 2, (1024, 2048, 8192))),
]


@gpu
@pytest.mark.parametrize("layouts", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("name,levels,m,l,n,families,plan", STRASSEN, ids=[s[0] for s in STRASSEN])
def test_mul_dev_strassen_on_views(dev, L, name, levels, m, l, n, families, plan, layouts):
    """Under EE and WIDE (even strides, 16-byte-aligned bases: WIDE is a column range of a wider matrix, the layout of the peeled
    core) the Strassen passes must run on the caller's buffers; under the other triples the same calls give the same bits and
    leave the same neighbours alone, whichever way they run."""
    plan(dev, m, l, n, "strassen")
    seed = 400 + 10 * [s[0] for s in STRASSEN].index(name)
    call = lambda A, B, C, acc: dev.mul(A, B, C, accumulate=acc, algo="strassen", param=levels)  # noqa: E731
    on_strassen = layouts in ((EE, EE, EE), (WIDE, WIDE, WIDE))
    run_products(dev, L, call, product(m, l, n, seed), (l, n, n), layouts, families if on_strassen else None, (name, m, l, n), seed)


@gpu
@pytest.mark.parametrize("which", [0, 1, 2], ids=["A", "B", "C"])
@pytest.mark.parametrize("levels,m,l,n", [(1, 128, 256, 256), (3, 512, 1024, 1024)])
def test_an_odd_ld_takes_the_plain_path(dev, L, levels, m, l, n, which):
    """include/m4ri_hip.h at gf2_mul_dev: "an odd `ld` takes the plain path instead of Strassen" -- with an odd `ld` on any one of
    A, B, C no gf2_strassen_ kernel launches (the level passes use 16-byte accesses on the operands they are given) and the product
    is right; with even strides and one base on an odd word the product is right whichever way it runs.  (From 1024 rows on a
    product that loses its levels this way may run them on zero-padded copies instead: the "padded" case above under the odd
    triples.)"""
    assert mul_plan(dev, m, l, n, "strassen", levels)[:2] == (levels, 0)
    call = lambda A, B, C, acc: dev.mul(A, B, C, accumulate=acc, algo="strassen", param=levels)  # noqa: E731
    ops = product(m, l, n, 400 + 10 * (levels - 1))
    for odd in (OE, OO):
        layouts = tuple(odd if k == which else EE for k in range(3))
        for ran in run_products(dev, L, call, ops, (l, n, n), layouts, None, ("odd ld", m, l, n), 50 + which):
            assert ran and not any("gf2_strassen_" in k for k in ran), (layouts, ran)
    layouts = tuple(EO if k == which else EE for k in range(3))
    run_products(dev, L, call, ops, (l, n, n), layouts, None, ("odd base", m, l, n), 60 + which)


# ---- gf2_mul_nt_dev ---------------------------------------------------------------------------------------------------------------

NT_M = 515   # three workgroups of 256 rows, the last one partial
# inner widths of 1, 2, 3, 4, 5, 8 and 9 words: every gf2_rowparity_kernel<WL> (1, 2, 4, 8 words in registers: 3 words run in <4>,
# 5 in <8>, with the registers past the row width cleared; 9 in the loop form <0>), four of the seven with a masked last word
NT_L = [37, 128, 191, 256, 257, 512, 513]
NT_N = [1, 64, 65, 130]


def rowparity_instance(l, a_layout):
    """the instantiation gf2k_rowparity picks: 16-byte loads of A need an even `ld` and a 16-byte-aligned base; the rest is 8-byte"""
    wl = g.width(l)
    if wl == 1:
        return 1
    if a_layout not in (EE, WIDE):
        return 0
    return 2 if wl <= 2 else 4 if wl <= 4 else 8 if wl <= 8 else 0


@gpu
@pytest.mark.parametrize("layouts", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("n", NT_N)
@pytest.mark.parametrize("l", NT_L)
def test_mul_nt_dev_row_widths_on_views(dev, L, l, n, layouts):
    call = lambda A, Bt, C, acc: dev.mul_nt(A, Bt, C, accumulate=acc)  # noqa: E731
    fam = "gf2_rowparity_kernelILi%dEE" % rowparity_instance(l, layouts[0])
    run_products(dev, L, call, product_nt(NT_M, l, n, 700 + l), (l, l, n), layouts, [fam], ("nt", NT_M, l, n), 70 + n)


# the wave-per-row form of gf2_mul_nt_dev in two passes (33-64 vectors), the second from Bt->data + 32 * Bt->ld into bits 32.. of
# C's word: one workgroup (5 rows: widevec_shape's rule for m <= 8) and many (its rule for 33-64 vectors)
NT_WIDEVEC = [(5, 8193, 33), (8193, 16385, 40)]


@gpu
@pytest.mark.parametrize("layouts", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("m,l,n", NT_WIDEVEC)
def test_mul_nt_dev_wave_per_row_on_views(dev, L, m, l, n, layouts):
    # no query reports widevec_shape alone: the census decides (a pass of 32 vectors, then one of the rest, and no row-parity kernel)
    call = lambda A, Bt, C, acc: dev.mul_nt(A, Bt, C, accumulate=acc)  # noqa: E731
    fams = ["gf2_widevec_kernelILi32E", "gf2_widevec_kernelILi%dE" % (1 if n == 33 else 8)]
    ran = run_products(dev, L, call, product_nt(m, l, n, 800 + m % 89), (l, l, n), layouts, fams, ("nt widevec", m, l, n), 80)
    assert not any("gf2_rowparity" in k for r in ran for k in r), ("no longer the wave-per-row path: pick another shape", ran)


# ---- gf2_transpose_dev ------------------------------------------------------------------------------------------------------------

# gf2_transpose512_kernel takes over from 2^29 bits on (gf2k_transpose): 8193 x 65537 is the smallest shape of the kind "one row
# above a multiple of its 512-row tiles, one column above a multiple of 64" that has them
TRANSPOSES = [(130, 70, "gf2_transpose_kernel"), (513, 2049, "gf2_transpose_kernel"), (8193, 65537, "gf2_transpose512_kernel")]


@gpu
@pytest.mark.parametrize("layouts", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("m,n,family", TRANSPOSES, ids=["%dx%d" % t[:2] for t in TRANSPOSES])
def test_transpose_dev_on_views(dev, L, m, n, family, layouts):
    import torch
    assert (m * n >= 1 << 29) == (family == "gf2_transpose512_kernel"), "the threshold of gf2k_transpose: pick another shape"
    s, want = transposed(m, n, 900 + m % 97)
    S = View(dev, m, n, layouts[0], 91, s)
    D = View(dev, n, m, layouts[1], 92)
    torch.cuda.synchronize()
    k0 = census(L)
    dev.transpose(S.m, D.m)
    torch.cuda.synchronize()
    k1 = census(L)
    check_c(D, want, ("transpose", m, n, layouts))
    S.unchanged("S")
    assert_route(k0, k1, [family])
