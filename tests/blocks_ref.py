"""Reference for the device block calls (gf2_copy_block_dev, gf2_submatrix_dev, gf2_concat_dev, gf2_stack_dev), in numpy on unpacked
bits, and the list of cases that tests/test_blocks_ref.py (host, no device) and tests/test_gpu_blocks.py share.  Nothing here calls
the library under test."""
import collections

import numpy as np

import gf2util as g


def copy_block(d_words, d_ncols, dr, dc, s_words, s_ncols, sr, sc, nrows, ncols, accumulate):
    """the words of D after D[dr+i][dc+j] (^)= S[sr+i][sc+j], i < nrows, j < ncols; d_words is (rows, width(d_ncols))"""
    d = g.words_to_bits(np.ascontiguousarray(d_words), d_ncols).copy()
    s = g.words_to_bits(np.ascontiguousarray(s_words), s_ncols)
    block = s[sr:sr + nrows, sc:sc + ncols]
    assert block.shape == (nrows, ncols) and dr + nrows <= d.shape[0] and dc + ncols <= d_ncols
    if accumulate:
        d[dr:dr + nrows, dc:dc + ncols] ^= block
    else:
        d[dr:dr + nrows, dc:dc + ncols] = block
    return g.bits_to_words(d) if d_ncols else np.zeros((d.shape[0], 0), dtype=np.uint64)


def submatrix(s_words, s_ncols, lowr, lowc, highr, highc):
    s = g.words_to_bits(np.ascontiguousarray(s_words), s_ncols)
    return g.bits_to_words(np.ascontiguousarray(s[lowr:highr, lowc:highc]))


def concat(a_words, a_ncols, b_words, b_ncols):
    a, b = g.words_to_bits(np.ascontiguousarray(a_words), a_ncols), g.words_to_bits(np.ascontiguousarray(b_words), b_ncols)
    return g.bits_to_words(np.hstack([a, b]))


def stack(a_words, b_words, ncols):
    a, b = g.words_to_bits(np.ascontiguousarray(a_words), ncols), g.words_to_bits(np.ascontiguousarray(b_words), ncols)
    return g.bits_to_words(np.vstack([a, b]))


Case = collections.namedtuple("Case", "d_rows d_ncols dr dc s_rows s_ncols sr sc nrows ncols accumulate seed")

OFFSETS = (0, 1, 31, 32, 33, 63)
WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 200)
ROWS = (1, 64, 65, 257)
# A (rows, cols), B (rows, cols) of the wrapper tests: concat shifts B by 36 bits; aligned; one bit
CONCATS = (((70, 100), (70, 29)), ((65, 64), (65, 64)), ((1, 1), (1, 1)))
STACKS = (((3, 130), (66, 130)), ((65, 64), (65, 64)), ((1, 1), (1, 1)))


def offset_grid():
    """source offset mod 64 x destination offset mod 64 x width x plain / accumulate, three rows; each offset gets 0 or 64 added
    (every combination of even and odd word positions occurs for every pair of offsets mod 64 across the widths), and the matrices
    end at the rectangle's last column in some cases and go on past it in others"""
    out = []
    for i, so in enumerate(OFFSETS):
        for j, do in enumerate(OFFSETS):
            for k, nc in enumerate(WIDTHS):
                for acc in (0, 1):
                    sc, dc = so + 64 * (k & 1), do + 64 * ((k >> 1) & 1)
                    s_ncols = sc + nc + (0 if (i + k) % 3 == 0 else 70)
                    d_ncols = dc + nc + (0 if (j + k) % 2 == 0 else 45)
                    out.append(Case(6, d_ncols, 2, dc, 5, s_ncols, 1, sc, 3, nc, acc, 1000 + len(out)))
    return out


def row_cases():
    """130 columns at offsets (5, 59): the partition of the rows among the threads"""
    return [Case(nr + 3, 59 + 130 + 11, 2, 59, nr + 1, 5 + 130, 1, 5, nr, 130, acc, 5000 + nr + acc) for nr in ROWS for acc in (0, 1)]


def cases():
    return offset_grid() + row_cases()


def operands(c):
    """(S words, dirty D words) of a case: random bits everywhere, the excess bits of the last words zero"""
    return g.random_words(c.s_rows, c.s_ncols, c.seed), g.random_words(c.d_rows, c.d_ncols, c.seed + 77777)


def expected(c):
    s, d = operands(c)
    return copy_block(d, c.d_ncols, c.dr, c.dc, s, c.s_ncols, c.sr, c.sc, c.nrows, c.ncols, c.accumulate)
