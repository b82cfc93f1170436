"""The LF1 kernels (m4ri-rust_amd/csrc/bkw/gf2_bkw.hip) read the key of a row through the shared reader alone (gf2_key_window /
gf2_row_key of csrc/gf2_dev_words.h).  tests/test_dev_words_cpu.py runs that reader on the CPU under the host compiler's address and
undefined-behaviour sanitizers, over every window [c0, c0 + b) with c0 + b <= ncols, b <= 30, for ncols in {1, 63, 64, 65, 128, 130}, on
rows whose heap block ends with the last word of the row, and again on a block that holds only the words with a bit of the window: the
cases that ran here while the file had a reader of its own.  No device is needed."""
import os

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "bkw", "gf2_bkw.hip")


def test_the_key_reads_only_the_words_of_the_window():
    text = open(KERNEL).read()
    shipped = kt.mask(text)
    # the kernels read the key through this function alone: no word of the window is named in this file
    assert shipped.count("gf2_row_key(") == 2     # the class firsts, the survivor rule of count and scatter
    assert shipped.count("gf2_key_window(") == 3  # the three kernels that read keys
    assert "w.w0" not in shipped and "w.mask" not in shipped and "lf1_key" not in shipped
    assert not kt._definitions(text, "gf2_row_key") and not kt._definitions(text, "gf2_key_window")
