"""Bodies of the child processes of tests/test_gpu_shipped_switches.py.  A child is started with one setting of the shipped
library's environment variables (most of them are read once per process) and runs `run(case)`: it shows that the setting took
effect -- the plan queries (no device needed) read at run time, and the launch census before and after every product -- and
compares the bits of every product with the C oracle, plain and accumulate form.  Nothing here sets a variable: the parent does."""
import ctypes
import json
import os
import re
import sys

import numpy as np

import gf2util as g
from census_util import census

import m4ri_rust_amd as pkg
from m4ri_rust_amd import _lib, device

L = _lib.lib()

# kernel family of every accepted M4RI_HIP_M4RM_CFG value, as it appears in the mangled kernel names of the census
FAMILY = {7: "gf2_m4rm_kernel_v3ILi8ELi128E", 20: "gf2_m4rm_kernel_v3ILi4ELi64E", 8: "gf2_m4rm_kernel_v6ILi8ELi4E",
          81: "gf2_m4rm_kernel_v6ILi8ELi6E", 82: "gf2_m4rm_kernel_v6ILi8ELi3E", 9: "gf2_m4rm_kernel_v8ILi8ELi2E",
          10: "gf2_m4rm_kernel_v8ILi4ELi2E", 11: "gf2_m4rm_kernel_v8ILi2ELi2E", 12: "gf2_m4rm_kernel_v8ILi1ELi2E"}
V8 = (9, 10, 11, 12)
READS_PACKED = (8, 9, 10, 11, 12)  # gf2_variants.h: who takes A row-group packed
TILE, PACK, STREAMK_REDUCE, SPLITK_REDUCE = "gf2_m4rm_kernel_", "gf2_packA_kernel", "gf2_streamk_reduce_kernel", "gf2_splitk_reduce_kernel"

PACKED_TILE = re.compile(r"gf2_m4rm_kernel_v8ILi\dELi2ELi1E|gf2_m4rm_kernel_v6ILi8ELi4ELi0ELi1E")  # the instantiations that read A row-group packed

PLAIN_SHAPES = [(300, 520, 2300), (4160, 1000, 1100), (600, 4096, 600), (1024, 1024, 70000)]
LONG_INNER, PACKS_A = (600, 4096, 600), (1024, 1024, 70000)
STRASSEN_SHAPES = [(1024, 1024, 1024, 1), (2048, 1024, 1536, 2), (1030, 2049, 2050, 1)]
PADDED = {(1030, 2049, 2050, 1): (1152, 2304, 2304)}  # rows to 64 << L, widths to 128 << L


# ---- the plan queries ----------------------------------------------------------------------------------

def tile_plan(m, l, n, batch=1, packed=0):
    out = (ctypes.c_longlong * 9)()
    t = L.gf2_tile_plan(m, l, n, batch, packed, out)
    tp = dict(zip(("cfg", "ksplit", "n_rem", "nseg", "scratch", "tail_batch", "tail_cfg", "tail_n_rem", "tail_nseg"), [int(v) for v in out]))
    band = (ctypes.c_longlong * 5)()
    L.gf2_tile_plan_band(m, l, n, batch, packed, band)
    tp.update(band_rows=int(band[0]), band_cfg=int(band[1]), t=t)
    return tp


def mul_plan(m, l, n, algo, param=0):
    kind, dims = ctypes.c_int(0), (ctypes.c_int * 3)()
    lv = L.gf2_mul_plan(m, l, n, device.ALGOS[algo], param, ctypes.byref(kind), dims)
    return int(lv), int(kind.value), tuple(int(d) for d in dims)


def workspace(m, l, n, algo, param=0):
    return int(L.gf2_mul_workspace_bytes(m, l, n, device.ALGOS[algo], param))


def leaf_tile_plan(dims, lv, packed):
    """the batched leaf launch of an lv-level product of the (padded) shape `dims`, as the planner sees it"""
    return tile_plan(dims[0] >> lv, dims[1] >> lv, dims[2] >> lv, 7 ** lv, packed)


def plans_of_every_shape():
    """what the parent compares with its own (default) answers"""
    out = {}
    for (m, l, n) in PLAIN_SHAPES:
        tp = tile_plan(m, l, n)
        tp.pop("t")
        out["%dx%dx%d" % (m, l, n)] = [tp, workspace(m, l, n, "m4rm")]
    for (m, l, n, p) in STRASSEN_SHAPES:
        out["%dx%dx%d/%d" % (m, l, n, p)] = [list(mul_plan(m, l, n, "strassen", p)), workspace(m, l, n, "strassen", p)]
    return out


# ---- products against the oracle -----------------------------------------------------------------------

def oracle_product(a, b, m, l, n):
    return (g.o_mul_fast if max(m, l, n) >= 4096 else g.o_mul_m4rm)(a, b, m, l, n)


def launched(before, after):
    return sorted(k for k, v in after.items() if v > before.get(k, 0))


def assert_clean(words, n, what):
    if n % 64:
        assert not (words[:, -1] >> np.uint64(n % 64)).any(), "%s: excess bits of the result are not zero" % (what,)


_seed = [1000]


def product(m, l, n, algo, param=0):
    """C = A B and C0 ^= A B through device.mul against the oracle, bit for bit; -> the kernels the two calls launched"""
    _seed[0] += 3
    s = _seed[0]
    a, b, c0 = g.random_words(m, l, s), g.random_words(l, n, s + 1), g.random_words(m, n, s + 2)
    ref = oracle_product(a, b, m, l, n)
    A, B = device.DMat.from_words(a, l), device.DMat.from_words(b, n)
    what = (m, l, n, algo, param)
    c_before = census(L)
    C = device.mul(A, B, algo=algo, param=param)
    got = C.to_words()
    ran = launched(c_before, census(L))
    assert_clean(got, n, what)
    bad = np.argwhere(got != ref)
    assert not len(bad), "%s: %d wrong words, first at %s" % (what, len(bad), tuple(bad[0]))
    C0 = device.DMat.from_words(c0, n)
    c_before = census(L)
    device.mul(A, B, C=C0, accumulate=True, algo=algo, param=param)
    got = C0.to_words()
    ran = sorted(set(ran) | set(launched(c_before, census(L))))
    assert_clean(got, n, what + ("accumulate",))
    bad = np.argwhere(got != (ref ^ c0))
    assert not len(bad), "%s accumulate: %d wrong words, first at %s" % (what, len(bad), tuple(bad[0]))
    return ran


def tiles_of(ran):
    return [k for k in ran if TILE in k]


def assert_family(ran, cfg, what):
    tk = tiles_of(ran)
    assert tk and all(FAMILY[cfg] in k for k in tk), "%s: variant %d was planned, tile kernels launched: %s" % (what, cfg, tk)


def has(ran, family):
    return any(family in k for k in ran)


def packed_tiles(ran):
    return [k for k in ran if PACKED_TILE.search(k)]


def plain_plans(m, l, n):
    """the plans a plain product may run: A as given, or packed first (plain_plan takes the faster one by its model)"""
    return [tile_plan(m, l, n, 1, 0), tile_plan(m, l, n, 1, 1)]


def assert_planned_families(ran, plans, what):
    """every tile kernel that launched belongs to a variant one of the plans names (main launch, tail launch or row band)"""
    cfgs = set()
    for p in plans:
        cfgs.add(p["cfg"])
        if p["tail_batch"] > 0:
            cfgs.add(p["tail_cfg"])
        if p["band_rows"] > 0:
            cfgs.add(p["band_cfg"])
    tk = tiles_of(ran)
    assert tk and all(any(FAMILY[c] in k for c in cfgs) for k in tk), "%s: variants %s were planned, tile kernels launched: %s" % (what, sorted(cfgs), tk)
    assert has(ran, PACK) == bool(packed_tiles(ran)), "%s: packing pass and packed tile kernels do not go together: %s" % (what, ran)


def strassen_case(m, l, n, param, algo="strassen", want_kind=None):
    """a product with Strassen levels: -> (levels, kind, dims, launched kernels); the leaf batch ran the planned family"""
    lv, kind, dims = mul_plan(m, l, n, algo, param)
    if want_kind is not None:
        assert kind == want_kind, (m, l, n, algo, param, lv, kind, dims)
    ran = product(m, l, n, algo, param)
    if lv > 0:
        assert has(ran, "gf2_strassen_"), ((m, l, n, param), ran)
        assert has(ran, "gf2_padcopy_kernel") == (kind == 1), ((m, l, n, param), kind, ran)
    else:
        assert not has(ran, "gf2_strassen_") and not has(ran, "gf2_padcopy_kernel"), ((m, l, n, param), ran)
    return lv, kind, dims, ran


# ---- M4RI_HIP_M4RM_CFG ---------------------------------------------------------------------------------

def case_cfg():
    """one accepted variant forced: every plan names it, only its kernel family launches, the bits are the oracle's"""
    cfg = int(os.environ["M4RI_HIP_M4RM_CFG"])
    for (m, l, n) in PLAIN_SHAPES:
        tp = tile_plan(m, l, n)
        assert tp["cfg"] == cfg and tp["tail_batch"] == 0 and tp["band_rows"] == 0, tp
        if (m, l, n) == LONG_INNER:  # few tiles, a long inner dimension: split-K, or every tile cut into segments
            if cfg in V8:
                assert tp["n_rem"] > 0 and tp["nseg"] > tp["n_rem"] and tp["scratch"] > 0, tp
            else:
                assert tp["ksplit"] > 1 and tp["scratch"] > 0, tp
        if cfg not in READS_PACKED:  # a packed request is refused: the plan that comes back is unpacked and carries no split
            pk = tile_plan(m, l, n, 1, 1)
            assert pk["cfg"] == cfg and pk["scratch"] == 0 and pk["ksplit"] == 1, pk
        ran = product(m, l, n, "m4rm")
        assert_family(ran, cfg, (m, l, n))
        assert has(ran, PACK) == bool(packed_tiles(ran)), ran
        run = plain_plans(m, l, n)[1] if has(ran, PACK) else tp  # (the variants that read packed A may take the packed plan)
        assert has(ran, STREAMK_REDUCE) == (cfg in V8 and run["n_rem"] > 0), (run, ran)
        assert has(ran, SPLITK_REDUCE) == (cfg not in V8 and run["ksplit"] > 1), (run, ran)
        if cfg not in READS_PACKED:
            assert not has(ran, PACK), ((m, l, n), ran)
    for (m, l, n, p) in STRASSEN_SHAPES:
        want = PADDED.get((m, l, n, p))
        lv, kind, dims, ran = strassen_case(m, l, n, p, want_kind=1 if want else 0)
        assert lv == p and (want is None or dims == want), (lv, kind, dims)
        assert_family(ran, cfg, (m, l, n, p))
        if cfg not in READS_PACKED:  # the leaves stay row-major; what the older kernels do with a batch: a uniform split-K
            leaf = leaf_tile_plan(dims, lv, 0)
            assert leaf["cfg"] == cfg, leaf
            assert has(ran, SPLITK_REDUCE) == (leaf["ksplit"] > 1), (leaf, ran)


def case_cfg_ignored():
    """a value outside the accepted list: the message (the parent reads stderr), and the default's plans (the parent compares) and bits"""
    for (m, l, n) in PLAIN_SHAPES:
        ran = product(m, l, n, "m4rm")
        assert_planned_families(ran, plain_plans(m, l, n), (m, l, n))
        if (m, l, n) == PACKS_A:
            assert has(ran, PACK), ran  # the default plan of this shape packs A: what the forced older variants must refuse
    for (m, l, n, p) in STRASSEN_SHAPES:
        strassen_case(m, l, n, p)


# ---- M4RI_HIP_APACK, M4RI_HIP_PLAIN_APACK --------------------------------------------------------------

def case_apack0():
    """Strassen leaves of A stay row-major: the leaf batch is the UNPACKED plan of the leaf shape, whatever that variant is, and
    no tile kernel that reads the packed layout launches (the last split pass writes that layout; no kernel of its own tells)"""
    for (m, l, n, p) in STRASSEN_SHAPES + [(2048, 2048, 2048, 3)]:
        want = PADDED.get((m, l, n, p))
        lv, kind, dims, ran = strassen_case(m, l, n, p, want_kind=1 if want else 0)
        assert lv == p, (lv, kind, dims)
        leaf = leaf_tile_plan(dims, lv, 0)
        assert_family(ran, leaf["cfg"], (m, l, n, p))
        assert not has(ran, PACK) and not packed_tiles(ran), ran
        if (m, l, n, p) == (2048, 2048, 2048, 3):
            assert leaf["cfg"] not in READS_PACKED, leaf  # 343 leaves of 256 rows: a variant no other test launches batched


def case_plain_apack0():
    """plain products never pack A first: no packing kernel, no packed copy in the workspace"""
    for (m, l, n) in [PACKS_A, (4608, 1024, 1024)]:
        tp = tile_plan(m, l, n)
        assert workspace(m, l, n, "m4rm") == tp["scratch"], (tp, workspace(m, l, n, "m4rm"))
        ran = product(m, l, n, "m4rm")
        assert not has(ran, PACK) and not packed_tiles(ran), ran
        assert_planned_families(ran, [tp], (m, l, n))


# ---- M4RI_HIP_SPLITK_WS_MIB (alone, with a forced variant, with the Strassen switches) -----------------

def unsplit_plain(m, l, n, cfg=None):
    plans = plain_plans(m, l, n)
    for tp in plans:
        assert tp["scratch"] == 0 and tp["ksplit"] == 1 and tp["n_rem"] == 0 and tp["nseg"] == 0 and tp["tail_n_rem"] == 0, tp
        assert cfg is None or tp["cfg"] == cfg, tp
    tp = plans[0]
    ran = product(m, l, n, "m4rm")
    assert_planned_families(ran, plans, (m, l, n))
    assert not has(ran, STREAMK_REDUCE) and not has(ran, SPLITK_REDUCE), ran
    return tp


def auto_case(m, l, n, levels=None, min_levels=None, kind=None):
    lv, k, dims, ran = strassen_case(m, l, n, 0, algo="auto", want_kind=kind)
    assert levels is None or lv == levels, (m, l, n, lv, k, dims)
    assert min_levels is None or lv >= min_levels, (m, l, n, lv, k, dims)
    assert lv == 0 or not has(ran, STREAMK_REDUCE), ran  # (the leaf batch finds no scratch for partial tiles either)
    return lv, k, dims, ran


def case_splitk_ws():
    """a cap of 0 or 1 MiB rejects every stream-K / split-K candidate: whole unsplit tiles, no reduction kernel, and the automatic level choice moves"""
    for (m, l, n) in PLAIN_SHAPES:
        unsplit_plain(m, l, n)
    auto_case(4096, 4096, 4096, min_levels=1)
    auto_case(4100, 4100, 4100, min_levels=1, kind=1)
    auto_case(5000, 4000, 4100, min_levels=1, kind=1)


def case_splitk_ws_cfg():
    """... with a forced older variant on top: the query reports the unsplit launch that runs (it used to report the split it could not have)"""
    cfg = int(os.environ["M4RI_HIP_M4RM_CFG"])
    unsplit_plain(*LONG_INNER, cfg=cfg)
    lv, kind, dims, ran = auto_case(4096, 4096, 4096)
    assert_family(ran, cfg, "4096^3 auto")
    assert not has(ran, SPLITK_REDUCE), ran
    for packed in (0, 1):
        leaf = leaf_tile_plan(dims, lv, packed)
        assert leaf["cfg"] == cfg and leaf["ksplit"] == 1 and leaf["scratch"] == 0, leaf


def case_leaf_min_512():
    assert mul_plan(2048, 2048, 2048, "auto")[0] == 2
    auto_case(2048, 2048, 2048, levels=2, kind=0)
    auto_case(3000, 3000, 3000, levels=1, kind=1)


def case_leaf_min_4096():
    auto_case(4096, 4096, 4096, levels=0, kind=0)


def case_max_levels_1():
    """the cap holds for the automatic choice only: an explicit level count is honoured as given"""
    auto_case(2048, 2048, 2048, levels=1, kind=0)
    lv, kind, dims, ran = strassen_case(2048, 2048, 2048, 2, want_kind=0)
    assert lv == 2 and L.gf2_strassen_levels(2048, 2048, 2048, device.ALGO_STRASSEN, 2) == 2, lv


def case_max_levels_0():
    auto_case(4096, 4096, 4096, levels=0, kind=0)
    assert L.gf2_strassen_levels(4096, 4096, 4096, device.ALGO_AUTO, 0) == 0
    lv, kind, dims, ran = strassen_case(4096, 4096, 4096, 1, want_kind=0)
    assert lv == 1, lv


# ---- M4RI_HIP_STRASSEN_PAD -----------------------------------------------------------------------------

def case_pad0():
    """shapes that do not divide by the level plan are neither padded nor peeled: they keep the levels the shape as given allows (here
    none) and run plain -- no padding copy, no split or merge pass.  With M4RI_HIP_SPLITK_WS_MIB=1 on top, the automatic choice would pad
    5000 x 4000 x 4100 (tests/test_gpu_shipped_switches.py::test_no_scratch_for_partial_tiles asserts that plan)"""
    for (m, l, n, algo, param) in [(1030, 2049, 2050, "strassen", 1), (5000, 4000, 4100, "auto", 0)]:
        lv, kind, dims, ran = strassen_case(m, l, n, param, algo=algo, want_kind=0)
        as_given = L.gf2_strassen_levels(m, l, n, device.ALGOS[algo], param)  # the level choice alone, on the shape as given
        assert lv == as_given == 0 and dims == (m, l, n), (m, l, n, lv, as_given, kind, dims)
        assert tiles_of(ran), ran
        assert workspace(m, l, n, algo, param) == workspace(m, l, n, "m4rm"), (m, l, n)
    if "M4RI_HIP_SPLITK_WS_MIB" in os.environ:  # a shape that divides keeps its automatic levels: only padding and peeling are off
        auto_case(4096, 4096, 4096, min_levels=1, kind=0)


# ---- the host-side switches: the mzd_* entries on host matrices ----------------------------------------

def host_product(entry, m, l, n, acc=False, rows=None, seed=7):
    a, b = g.random_words(m, l, seed), g.random_words(l, n, seed + 1)
    A, B = pkg.BinMatrix.from_words(a, l), pkg.BinMatrix.from_words(b, n)
    c0 = g.random_words(m, n, seed + 2) if acc else None
    C = pkg.BinMatrix.from_words(c0, n) if acc else None
    args = (C.mzd if acc else None, A.mzd, B.mzd) + ((0,) if "m4rm" in entry else ())
    out = getattr(L, entry)(*args)
    assert out, entry
    got = C.to_words() if acc else pkg.BinMatrix(out).to_words()
    assert_clean(got, n, (entry, m, l, n))
    if rows is None:
        ref = oracle_product(a, b, m, l, n)
    else:  # a sample of rows: the oracle on those rows of A
        ref, got = oracle_product(np.ascontiguousarray(a[rows]), b, len(rows), l, n), got[rows]
        c0 = c0[rows] if acc else None
    bad = np.argwhere(got != (ref ^ c0 if acc else ref))
    assert not len(bad), "%s %s: %d wrong words, first at %s" % (entry, (m, l, n), len(bad), tuple(bad[0]))


def case_pipeline_blocks():
    """the thin pipeline: A is exactly 8 MiB and the rows divide by 64 * blocks for every block count"""
    for entry in ("mzd_mul_m4rm", "mzd_mul_naive"):
        host_product(entry, 65536, 1024, 64)
    for entry in ("mzd_addmul_m4rm", "mzd_addmul_naive"):
        host_product(entry, 65536, 1024, 64, acc=True)


def case_pipeline_big():
    n = 16384
    rows = np.unique(np.concatenate([np.array([0, 1, 63, 64, n // 2 - 1, n // 2, n - 1]), (np.arange(200, dtype=np.int64) * 7919 + 13) % n]))
    host_product("mzd_mul_m4rm", n, n, n, rows=rows)
    host_product("mzd_addmul_m4rm", n, n, n, acc=True, rows=rows)


def dirty_parent(nrows, ncols, seed):
    """random bits in every word of every row, the excess bits of the last word included (tests/test_gpu_views.py)"""
    P = pkg.BinMatrix.from_words(g.random_words(nrows, ncols, seed), ncols)
    w = g.width(ncols)
    P._words_view()[:, :w] = g.splitmix64(seed ^ 0xD1B54A32D192ED03, np.arange(nrows * w, dtype=np.uint64)).reshape(nrows, w)
    return P


def case_transpose():
    """every mzd_transpose on the device (threshold 1 bit) against numpy's transpose of the bits"""
    R0, C0 = 5, 64
    for (r, c) in [(1, 1), (1, 70), (70, 1), (64, 64), (65, 127), (129, 300)]:
        src = g.random_words(r, c, 31 * r + c)
        want = g.bits_to_words(np.ascontiguousarray(g.words_to_bits(src, c).T))
        S = pkg.BinMatrix.from_words(src, c)
        # a NULL destination
        before = census(L)
        out = L.mzd_transpose(None, S.mzd)
        assert out and has(launched(before, census(L)), "gf2_transpose"), (r, c)
        got = pkg.BinMatrix(out).to_words()
        assert_clean(got, r, (r, c, "NULL destination"))
        assert np.array_equal(got, want), (r, c, "NULL destination")
        # a given plain destination, dirty before the call
        D = pkg.BinMatrix.from_words(g.random_words(c, r, 5), r)
        before = census(L)
        assert L.mzd_transpose(D.mzd, S.mzd)
        assert has(launched(before, census(L)), "gf2_transpose"), (r, c)
        got = D.to_words()
        assert_clean(got, r, (r, c, "plain destination"))
        assert np.array_equal(got, want), (r, c, "plain destination")
        # the source a window at (5, 64) of a dirty parent: the parent comes back unchanged
        pc = C0 + c + 70
        P = dirty_parent(R0 + r + 3, pc, 77 + r)
        raw = g.words_to_bits(P.to_words(), g.width(pc) * 64)
        W = L.mzd_init_window(P.mzd, R0, C0, R0 + r, C0 + c)
        want_w = g.bits_to_words(np.ascontiguousarray(raw[R0:R0 + r, C0:C0 + c].T))
        before = census(L)
        out = L.mzd_transpose(None, W)
        assert out and has(launched(before, census(L)), "gf2_transpose"), (r, c)
        got = pkg.BinMatrix(out).to_words()
        assert_clean(got, r, (r, c, "source window"))
        assert np.array_equal(got, want_w), (r, c, "source window")
        assert np.array_equal(g.words_to_bits(P.to_words(), g.width(pc) * 64), raw), (r, c, "the source's parent changed")
        L.mzd_free(W)
        # a destination window (the host path): right inside, every bit of its parent outside as it was
        pr = C0 + r + 70
        Q = dirty_parent(R0 + c + 3, pr, 99 + c)
        rawq = g.words_to_bits(Q.to_words(), g.width(pr) * 64)
        V = L.mzd_init_window(Q.mzd, R0, C0, R0 + c, C0 + r)
        assert L.mzd_transpose(V, S.mzd)
        expect = rawq.copy()
        expect[R0:R0 + c, C0:C0 + r] = g.words_to_bits(want, r)
        bad = np.argwhere(g.words_to_bits(Q.to_words(), g.width(pr) * 64) != expect)
        assert not len(bad), "%s destination window: %d wrong bits, first at %s" % ((r, c), len(bad), tuple(bad[0]))
        L.mzd_free(V)


def case_pinning():
    """host blocks pinned from 4 KiB on, never (2^40), or pinned but never kept after mzd_free (cache of 0 bytes): the library offers no
    public observable of where a block lives (gf2_mzd_block_is_pinned is internal), so the bits of the paths that treat pinned and
    pageable operands differently are compared, and a re-used block must come back zeroed"""
    m, l = 1 << 18, 256
    a = g.random_words(m, l, 41)
    A = pkg.BinMatrix.from_words(a, l)
    v = g.random_words(1, l, 42)
    for _ in range(2):  # (the second call finds what the first one freed)
        got = A.mul_slice(v[0]).to_words()
        ref = g.o_mul_m4rm(a, g.bits_to_words(np.ascontiguousarray(g.words_to_bits(v, l).T)), m, l, 1)
        assert np.array_equal(got, ref), "A * v"
    del A
    host_product("mzd_mul_naive", m, l, 3, seed=43)
    host_product("mzd_addmul_naive", m, l, 3, acc=True, seed=43)
    host_product("mzd_mul_m4rm", 16384, 256, 64, seed=46)
    host_product("mzd_addmul_m4rm", 16384, 256, 64, acc=True, seed=46)
    for _ in range(2):
        M = pkg.BinMatrix.zero(4096, 4096)  # 2 MiB
        assert not M._words_view().any(), "mzd_init: not zero"
        M._words_view()[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
        del M
        M = pkg.BinMatrix.zero(4096, 4096)
        assert not M._words_view().any(), "mzd_init after mzd_free of a filled matrix: not zero"
        del M


CASES = {f.__name__[5:]: f for f in (case_cfg, case_cfg_ignored, case_apack0, case_plain_apack0, case_splitk_ws, case_splitk_ws_cfg, case_leaf_min_512,
                                     case_leaf_min_4096, case_max_levels_1, case_max_levels_0, case_pad0, case_pipeline_blocks, case_pipeline_big,
                                     case_transpose, case_pinning)}


def run(case):
    device.require_gpu()
    CASES[case]()
    print("SWITCH-PLANS " + json.dumps(plans_of_every_shape(), sort_keys=True))
    print("SWITCH-OK " + case)
    sys.stdout.flush()
