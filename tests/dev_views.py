"""Operands of the device-resident entries as 8-byte-aligned views of a caller's buffer (tests/test_gpu_mul_views.py).

A view is a window of a parent that holds random bits in every word outside the window: at least one row above and two rows below it,
at least one word left and right of it, and the words between the row width and `ld`.  The window itself holds clean words (zero
excess bits in the last word: what gf2_dmat promises for A, B and C).  A kernel that reads one word too far computes with random
bits, and one that writes one word too far, or drops the mask of the last word, changes a word that expect() / unchanged() compare.

Layouts: (is `ld` odd, does the window start on an odd word) -- 16-byte accesses are possible only where both are even --, and WIDE:
an even `ld` of at least twice the row width behind a 16-byte-aligned base, a column range of a wider matrix.

geometry() and parent_words() are plain numpy; View needs torch, and a device only when it is given the device module."""
import numpy as np

import gf2util as g

EE, EO, OE, OO, WIDE = "EE", "EO", "OE", "OO", "WIDE"
LAYOUTS = (EE, EO, OE, OO, WIDE)
_PARITY = {EE: (False, False), EO: (False, True), OE: (True, False), OO: (True, True), WIDE: (False, False)}

R0 = 1      # rows of the parent above the window
BELOW = 2   # rows of the parent below it


def geometry(ncols, layout):
    """-> (ld, cw): the parent's row stride and the window's first word within a row, both in 64-bit words"""
    ld_odd, base_odd = _PARITY[layout]
    w = g.width(ncols)
    if layout == WIDE:
        ld = 2 * w + 2
        cw = 2
    else:
        ld = w + 3
        if bool(ld & 1) != ld_odd:
            ld += 1
        cw = 1 if bool((R0 * ld + 1) & 1) == base_odd else 2
    assert bool(ld & 1) == ld_odd and bool((R0 * ld + cw) & 1) == base_odd, (ncols, layout, ld, cw)
    assert cw >= 1 and ld - cw - w >= 1 and (layout != WIDE or ld >= 2 * w), (ncols, layout, ld, cw)
    return ld, cw


def parent_words(nrows, ncols, layout, seed, words=None):
    """-> the parent as (R0 + nrows + BELOW) x ld uint64: random words, `words` (default: seeded clean random words) in the window"""
    ld, cw = geometry(ncols, layout)
    w = g.width(ncols)
    host = np.random.default_rng(seed).integers(0, 1 << 64, (R0 + nrows + BELOW, ld), dtype=np.uint64)
    if words is None:
        words = g.random_words(nrows, ncols, seed ^ 0x5EED)
    assert words.shape == (nrows, w) and words.dtype == np.uint64, (words.shape, nrows, w)
    if ncols % 64 and nrows:
        assert not (words[:, -1] >> np.uint64(ncols % 64)).any(), "the window's words must have zero excess bits"
    host[R0:R0 + nrows, cw:cw + w] = words
    return host


class View:
    """nrows x ncols in the given layout.  dev: the device module (m4ri_rust_amd.device): the parent goes to the GPU and `m` is the
    gf2_dmat of the window; None: the parent stays a CPU tensor and `m` is None (the layout claims can be checked without a GPU)."""

    def __init__(self, dev, nrows, ncols, layout, seed, words=None):
        import torch
        self.nrows, self.ncols, self.layout = nrows, ncols, layout
        self.ld, self.cw = geometry(ncols, layout)
        self.w = g.width(ncols)
        self.host = parent_words(nrows, ncols, layout, seed, words)
        self.host.setflags(write=False)
        t = torch.from_numpy(self.host.view(np.int64).copy())
        self.t = t.cuda() if dev is not None else t
        ld_odd, base_odd = _PARITY[layout]
        self.base = self.t.data_ptr() + 8 * (R0 * self.ld + self.cw)
        assert self.t.data_ptr() % 16 == 0, "the parent is not 16-byte aligned"
        assert bool(self.ld & 1) == ld_odd and bool((self.base // 8) & 1) == base_odd and self.base % 8 == 0, (layout, self.ld, self.base)
        if layout == WIDE:
            assert self.ld >= 2 * self.w and self.base % 16 == 0
        self.m = dev.DMat.wrap(self.base, nrows, ncols, self.ld, keep=self.t) if dev is not None else None

    def window(self, parent=None):
        """the window's words of `parent` (default: as uploaded)"""
        p = self.host if parent is None else parent
        return p[R0:R0 + self.nrows, self.cw:self.cw + self.w]

    def read(self):
        """the whole parent as it is now"""
        return self.t.cpu().numpy().view(np.uint64).reshape(self.host.shape)

    def unchanged(self, name="an operand"):
        got = self.read()
        assert np.array_equal(got, self.host), "%s's parent changed, first at (row, word) %s" % (name, tuple(np.argwhere(got != self.host)[0]))

    def expect(self, rows):
        """the parent as uploaded, with only the window's width(ncols) words replaced by `rows`"""
        assert rows.shape == (self.nrows, self.w), (rows.shape, self.nrows, self.w)
        want = self.host.copy()
        want[R0:R0 + self.nrows, self.cw:self.cw + self.w] = rows
        return want
