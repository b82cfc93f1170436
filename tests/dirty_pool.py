"""Dirty internal scratch for tests/test_gpu_dirty_workspace.py: the memory the library hands to ITSELF.

Every entry point draws its scratch, the device copies of host operands and the results it allocates from one block cache
(gf2_dev_alloc in runtime_host.cpp: DevBuf, the per-stream arenas of gf2_stream_scratch, gf2_dmat_alloc), and nothing clears a block.
seed() empties that cache, refills it with blocks that hold a known pattern in every word and notes the allocation counters
(gf2_dev_alloc_counts): as long as the count of fresh hipMallocs stands still, every block a call used -- operands, results, scratch --
came from the seeded cache, so it held the pattern wherever the library had not written it.

The cache serves a request only from a block of 1 to 1.25 times its size rounded up to 1 MiB (below 64 MiB), so the seed list holds
every size from 1 to 8 MiB, plus what a case names in `extra` (its arenas and operands above 8 MiB).

Two patterns, always in this order within a case: INDEX (0x0000000100000001 in every word: non-zero as bits, and the in-range index 1
to a kernel that takes an unwritten word for an int), asserted first; RANDOM (the oracle's splitmix64 stream through
gf2_dmat_fill_random) only after the first pattern's assertions have passed.  A kernel that reads an index array it did not write
must show up as wrong bits under the first pattern, not as a wild address under the second."""
import ctypes
import time

import numpy as np

INDEX = 0x0000000100000001
RANDOM = "splitmix64"
PATTERNS = (INDEX, RANDOM)

MIB = 1 << 20
COLS = 8192                 # 1024 k rows x 8192 columns = k MiB exactly (ld = 128 words)
CHUNK_ROWS = 8 * 1024       # fills go up in pieces of 8 MiB
SIZES = [(k, 16) for k in range(1, 9)] + [(1, 32)]  # (MiB, copies)

_host_const = {}


def counts(L):
    """(requests served from the block cache, requests served by a fresh hipMalloc) since the library was loaded"""
    out = (ctypes.c_longlong * 2)()
    L.gf2_dev_alloc_counts(out)
    return int(out[0]), int(out[1])


def pad_word(pattern):
    """what a test writes into the pad word of an operand it uploads (the block's own content is lost to the upload)"""
    return INDEX if pattern == INDEX else 0xD1B54A32D192ED03


def _const_rows(rows, word):
    from m4ri_rust_amd import BinMatrix
    key = (rows, word)
    if key not in _host_const:
        _host_const[key] = BinMatrix.from_words(np.full((rows, COLS // 64), word, dtype=np.uint64), COLS)
    return _host_const[key]


def _fill_const(L, S, word):
    from m4ri_rust_amd._lib import DMatStruct, check
    for r0 in range(0, S.nrows, CHUNK_ROWS):
        rows = min(CHUNK_ROWS, S.nrows - r0)
        view = DMatStruct(S.data + 8 * r0 * S.ld, S.ld, rows, COLS)
        check(L.gf2_dmat_upload(ctypes.byref(view), _const_rows(rows, word).mzd, None), "gf2_dmat_upload")


def seed(L, pattern, extra=()):
    """Cache, arenas and deferred frees back to the driver (gf2_trim); then blocks of 1 .. 8 MiB (16 of each, 32 more of 1 MiB) and one
    of every size in `extra` (MiB) are allocated, filled with `pattern` in every word and freed into the cache.  -> seconds taken."""
    from m4ri_rust_amd._lib import DMatStruct, check
    t0 = time.perf_counter()
    check(L.gf2_trim(), "gf2_trim")
    blocks = []
    for mib, copies in SIZES + [(int(e), 1) for e in extra]:
        for _ in range(copies):
            S = DMatStruct()
            check(L.gf2_dmat_alloc(ctypes.byref(S), 1024 * mib, COLS), "gf2_dmat_alloc")
            assert S.ld * 8 * S.nrows == mib * MIB
            blocks.append(S)
    for i, S in enumerate(blocks):
        if pattern == INDEX:
            _fill_const(L, S, INDEX)
        else:
            check(L.gf2_dmat_fill_random(ctypes.byref(S), 0x5EED0000 + i, None), "gf2_dmat_fill_random")
    for S in blocks:
        L.gf2_dmat_free(ctypes.byref(S))
    return time.perf_counter() - t0


class Pool:
    """One seeded cache: Pool(L, pattern, extra) seeds; no_fresh() asserts that no block has come from the driver since."""

    def __init__(self, L, pattern, extra=()):
        self.L, self.pattern = L, pattern
        self.seed_seconds = seed(L, pattern, extra)
        self.hits0, self.fresh0 = counts(L)

    def hits(self):
        return counts(self.L)[0]

    def no_fresh(self, what=""):
        fresh = counts(self.L)[1] - self.fresh0
        assert fresh == 0, "%s: %d block(s) came fresh from the driver, not from the seeded cache" % (what, fresh)


def dmat(words, ncols, pad):
    """A device matrix from the cache holding `words` (nrows x width(ncols), zero excess bits) with `pad` in the pad word of its even
    row stride: the whole stride of every row goes up in one copy through a view that is ld words wide."""
    from m4ri_rust_amd import BinMatrix, device
    from m4ri_rust_amd._lib import check, lib
    words = np.ascontiguousarray(words, dtype=np.uint64)
    M = device.DMat(words.shape[0], ncols)
    full = np.full((words.shape[0], M.ld), pad, dtype=np.uint64)
    full[:, :words.shape[1]] = words
    view = device.DMat.wrap(M.s.data, M.nrows, M.ld * 64, M.ld)
    check(lib().gf2_dmat_upload(ctypes.byref(view.s), BinMatrix.from_words(full, M.ld * 64).mzd, None), "gf2_dmat_upload")
    M.full = full  # what the block holds now, for unchanged()
    return M


def unchanged(M, stream=None):
    """an operand made by dmat() still holds every word it was given, the pad word included"""
    assert np.array_equal(raw(M, stream), M.full), "an operand (or the pad word of its row stride) changed"


def raw(M, stream=None):
    """every word of every row of a device matrix or view, the pad word included: (nrows, ld)"""
    from m4ri_rust_amd import device
    view = device.DMat.wrap(M.s.data, M.nrows, M.ld * 64, M.ld)
    return view.to_words(stream)
