"""The word-level helpers that the LPN modules share (m4ri-rust_amd/csrc/gf2_dev_words.h) run on the CPU under the host compiler's
address and undefined-behaviour sanitizers (tests/dev_words_emu.cpp): the shipped text, cut out with tests/kernel_text.py, in a program
of its own.  These are the cases that the modules' tests ran on the modules' own copies of the helpers.

  gf2_key_window / gf2_row_key: every window [c0, c0 + b) with c0 + b <= ncols, b <= 30, for ncols in {1, 63, 64, 65, 128, 130}, on rows
  whose heap block ends with the last word of the row, and again on a block that holds only the words with a bit of the window.  Every
  key must equal the bit-by-bit definition; a read of a word that holds no bit of the window is a sanitizer report, which a GPU test
  could show only by faulting.
  gf2_word_mask / gf2_word_weight: the bits and the ones of a word in a column range, over every [wc0, wc1) of ncols in
  {1, 63, 64, 65, 130}, against the bits written out one by one.
  gf2_find_position: the position that an output of a run belongs to, on sums with empty positions, one giant position and 64-bit
  totals.

gf2_lo_hi and gf2_load2 run in tests/test_join_select_helpers_cpu.py, under the helper that calls them.  gf2_block_scan crosses lanes
and is not emulated; the GPU suites of lf2 and join run it.  The second test holds the layout: one copy of each shared piece.

No device is needed."""
import glob
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc")
HEADER = os.path.join(CSRC, "gf2_dev_words.h")
HELPERS = ["Gf2KeyWindow", "gf2_key_window", "gf2_row_key", "gf2_lo_hi", "gf2_load2", "gf2_word_mask", "gf2_word_weight", "gf2_find_position"]
SHARED = HELPERS[1:] + ["gf2_block_scan", "gf2_rows_aligned16"]
# the names that the modules' own copies had
FORMER = ["lf1_window", "lf1_key", "lf2_window", "lf2_key", "lf1_lo_hi", "lf2_lo_hi", "join_lo_hi", "sums_lo_hi", "weight_lo_hi", "gather_lo_hi",
          "lf2_find_position", "join_find_position", "join_word_weight", "sums_word_weight", "near_word_mask", "join_load2", "lf2_block_scan",
          "join_block_scan", "lf1_rows_aligned16", "lf2_rows_aligned16", "join_rows_aligned16", "sums_rows_aligned16", "weight_rows_aligned16"]
KEY_WIDTHS = (1, 63, 64, 65, 128, 130)
WIDTHS = (1, 63, 64, 65, 130)


def sources():
    found = [p for pat in ("*.h", "*.hip", "*.inc", "*.cpp") for p in glob.glob(os.path.join(CSRC, "**", pat), recursive=True)]
    assert HEADER in found and len(found) > 60
    return sorted(found)


def test_the_shared_helpers_on_the_cpu(tmp_path):
    body = tmp_path / "dev_words_body.inc"
    body.write_text(kt.extract_all(HEADER, HELPERS))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    exe = tmp_path / "dev_words_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "dev_words_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    windows = sum(1 for n in KEY_WIDTHS for c0 in range(n + 1) for b in range(31) if c0 + b <= n)
    assert "%d keys ok" % (3 * windows) in run.stdout, run.stdout
    ranges = sum(1 for n in WIDTHS for wc0 in range(n + 1) for wc1 in range(wc0, n + 1))
    assert "%d weights ok" % (3 * ranges) in run.stdout, run.stdout
    positions = re.search(r"(\d+) positions ok", run.stdout)
    assert positions and int(positions.group(1)) >= 1000, run.stdout


def test_every_shared_piece_has_one_home():
    """a helper that two modules use is defined in the header and nowhere else; the copies are gone"""
    header = kt.mask(open(HEADER).read())
    for name in SHARED + ["Gf2KeyWindow"]:
        kt.extract(HEADER, name)   # KeyError: none, ValueError: two
    # the window's words and the popcount of a ranged weight are named there and nowhere else
    assert header.count("w.w0") == 3 and header.count("__popcll(") == 1 and header.count("__shfl_up(") == 1
    for path in sources():
        if path == HEADER:
            continue
        text = kt.mask(open(path).read())
        assert "w.w0" not in text and "& 15) && (!(" not in text, path
        for name in SHARED + FORMER + ["Gf2KeyWindow", "Lf1Window", "Lf2Window"]:
            assert name not in text or not kt._definitions(open(path).read(), name), (path, name)
    assert header.count("& 15) && (!(") == 1
    # the header travels with the library's sources: named in LIB_HDR, once, and included by the kernel files alone
    mk = open(os.path.join(CSRC, "sources.mk")).read()
    assert mk.count("gf2_dev_words.h") == 1 and "gf2_dev_words.h" in mk[mk.index("LIB_HDR"):]
    users = [p for p in sources() if '#include "../gf2_dev_words.h"' in open(p).read()]
    assert len(users) >= 9 and all(p.endswith(".hip") for p in users), users
