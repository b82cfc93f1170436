"""CPU side of tests/test_gpu_limits.py: the shapes that cross the two limits, any rows or word columns of a seeded matrix without a
download, the sampled rows, row-range views and downloads through them, a one-word bit flip, the bit-offset reference of
gf2_copy_block_dev on sampled rows, and a plain numpy product for a long inner dimension.  Nothing here calls a kernel under test except gf2_dmat_download / _upload (plain copies)."""
import numpy as np

import gf2util as g

LIMIT_ROWS = 65536 * 64            # 4 194 304: the first row count whose 64-row blocks no longer fit a 16-bit launch dimension
LIMIT_BYTES = 1 << 32
R = LIMIT_ROWS + 65                # 65 537 whole 64-row blocks and one row
BIG_TALL = (9000001, 4096)         # ld 64 words, 4.6 GB: byte offset 2^32 is the start of row 8 388 608
BIG_WIDE = (36929, 1048640)        # ld 16 386 words (even, no power of two), 4.84 GB
PIECE_ROWS = 1 << 21               # whole-result checks: row blocks of at most 2^21 rows ...
PIECE_BYTES = 1 << 31              # ... and at most 2 GiB


def even(w):
    return (w + 1) & ~1


def seeded_words(seed, ncols, rows, words=None):
    """Words `words` (default: all) of rows `rows` of the matrix gf2_dmat_fill_random(seed) makes with ncols columns: word (r, j) is
    splitmix64(seed, r * width + j), the excess bits of the last word zero.  -> (len(rows), len(words)) uint64"""
    w = g.width(ncols)
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    words = np.arange(w, dtype=np.uint64) if words is None else np.asarray(words, dtype=np.uint64).reshape(-1)
    out = g.splitmix64(seed, rows[:, None] * np.uint64(w) + words[None, :])
    if ncols % 64:
        out[:, words == np.uint64(w - 1)] &= np.uint64((1 << (ncols % 64)) - 1)
    return np.ascontiguousarray(out)


def seeded_matrix(seed, nrows, ncols, chunk=1 << 20):
    """the whole seeded matrix, generated in row chunks (the temporaries of a 500 MB matrix would otherwise be several times its size)"""
    out = np.empty((nrows, g.width(ncols)), dtype=np.uint64)
    for r0 in range(0, nrows, chunk):
        r1 = min(nrows, r0 + chunk)
        out[r0:r1] = seeded_words(seed, ncols, np.arange(r0, r1, dtype=np.uint64))
    return out


def straddle(ld, nrows):
    """the two rows on either side of byte offset 2^32 in a matrix of row stride ld: the last that starts below it and the first that
    starts at or above it; () when the matrix ends before"""
    k = -(-LIMIT_BYTES // (8 * ld))
    return (k - 1, k) if k < nrows else ()


def sample_rows(nrows, ld, seed, count=200):
    """row 0 and the last; both sides of row 4 194 304 and of byte offset 2^32; first and last row of the last ragged 64-row block;
    `count` rows drawn with a fixed seed"""
    rows = {0, nrows - 1, (nrows - 1) // 64 * 64}
    if nrows > LIMIT_ROWS:
        rows |= {LIMIT_ROWS - 1, LIMIT_ROWS}
    rows |= set(straddle(ld, nrows))
    rows |= set(int(r) for r in np.random.default_rng(seed).integers(0, nrows, size=count))
    return np.array(sorted(rows), dtype=np.int64)


def row_view(dev, M, r0, nrows, ncols=None, word0=0):
    """rows [r0, r0 + nrows) of M from word column word0 on, as a view of the same buffer"""
    return dev.DMat.wrap(M.s.data + 8 * (r0 * M.ld + word0), nrows, M.ncols - 64 * word0 if ncols is None else ncols, M.ld, keep=M)


def fetch_rows(dev, M, rows, stream=None):
    """the given rows of a device matrix, downloaded through row-range views (runs of consecutive rows in one copy)"""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.empty((len(rows), g.width(M.ncols)), dtype=np.uint64)
    i = 0
    while i < len(rows):
        j = i + 1
        while j < len(rows) and rows[j] == rows[j - 1] + 1:
            j += 1
        out[i:j] = row_view(dev, M, int(rows[i]), j - i).to_words(stream)
        i = j
    return out


def flip_bit(pkg, dev, M, r, word, bit):
    """one bit of word (r, word) of a device matrix, through a download and an upload of that word alone"""
    import ctypes
    v = dev.DMat.wrap(M.s.data + 8 * (r * M.ld + word), 1, 64, 2, keep=M)
    w = v.to_words()
    w[0, 0] ^= np.uint64(1 << bit)
    pkg._lib.check(pkg._lib.lib().gf2_dmat_upload(ctypes.byref(v.s), pkg.BinMatrix.from_words(w, 64).mzd, None), "gf2_dmat_upload")


def pieces(nrows, ld, step=64):
    """row blocks [r0, r1) of at most 2^21 rows and 2 GiB, every r0 a multiple of `step`"""
    per = min(PIECE_ROWS, PIECE_BYTES // (8 * ld)) // step * step
    return [(r0, min(nrows, r0 + per)) for r0 in range(0, nrows, per)]


def shifted(a, ncols, shift, out_words):
    """rows of ncols bits moved up by `shift` (< 64) bits into rows of out_words words"""
    out = np.zeros((a.shape[0], out_words), dtype=np.uint64)
    w = g.width(ncols)
    out[:, :w] = a << np.uint64(shift)
    if shift:
        hi = a >> np.uint64(64 - shift)
        k = min(w, out_words - 1)
        out[:, 1:1 + k] |= hi[:, :k]
    return out


def block_at_offset(c0, a, ncols, shift, accumulate):
    """what gf2_copy_block_dev leaves in rows that held c0 when the ncols bits of the rows a go to bit offset `shift`"""
    ones = np.full((1, g.width(ncols)), ~np.uint64(0), dtype=np.uint64)
    if ncols % 64:
        ones[0, -1] = np.uint64((1 << (ncols % 64)) - 1)
    mask, sh = shifted(ones, ncols, shift, c0.shape[1]), shifted(a, ncols, shift, c0.shape[1])
    return c0 ^ sh if accumulate else (c0 & ~mask) | sh


def mul_rows_ref(a, b, l):
    """A B as the XOR of the rows of B that each row of A selects: plain numpy, for a long inner dimension and few rows of A"""
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.uint64)
    for i in range(a.shape[0]):
        out[i] = np.bitwise_xor.reduce(b[g.words_to_bits(a[i:i + 1], l)[0].astype(bool)], axis=0)
    return out
