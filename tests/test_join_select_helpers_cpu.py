"""The word-level helpers of the weight-filtered join (m4ri-rust_amd/csrc/join/gf2_join_select.inc) run on the CPU under the host
compiler's address and undefined-behaviour sanitizers (tests/join_select_emu.cpp), as tests/test_join_helpers_cpu.py does it for the
join: the shipped text, cut out with tests/kernel_text.py, in a program of its own.

  join_select_first_word / join_select_end_word: the words of a row that hold a column of [wc0, wc1), over every range of ncols in
  {1, 63, 64, 65, 130}: exactly the words that the definition names, and their weights sum to a bit-by-bit count.
  join_select_pair_weight: the ones of a ^ p on the range, dealt to 1, 2, 8 and 64 lanes, with 8-byte and with 16-byte accesses, on
  rows in heap blocks of exactly the row's words: no word behind the row is read.
  join_select_is_hit: every window 0 <= wlo <= whi <= width + 2 of every range.

No device is needed."""
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
JOIN = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "join")
KERNEL, SELECT = os.path.join(JOIN, "gf2_join.hip"), os.path.join(JOIN, "gf2_join_select.inc")
WORDS = os.path.join(os.path.dirname(JOIN), "gf2_dev_words.h")
SHARED = ["gf2_lo_hi", "gf2_load2", "gf2_word_weight"]             # of gf2_dev_words.h, called by the helpers
HELPERS = ["join_select_first_word", "join_select_end_word", "join_select_is_hit", "join_select_pair_weight"]
WIDTHS = (1, 63, 64, 65, 130)


def test_the_new_kernels_use_no_atomics_and_no_assembly():
    shipped = kt.mask(open(SELECT).read())
    assert "atomic" not in shipped and "asm" not in shipped
    assert kt.global_kernels(SELECT) == ["gf2_join_weigh_kernel", "gf2_join_select_scatter_kernel"]
    # both kernels weigh and test a pair through the helpers alone, and gf2_join.hip includes the file once, inside its namespace
    assert shipped.count("join_select_pair_weight(") == 3 and shipped.count("join_select_is_hit(") == 3
    assert shipped.count("__popcll(") == 2          # the ranking alone: a wave's hits, the hits before a group; weights go through gf2_word_weight
    text = open(KERNEL).read()
    assert text.count('#include "gf2_join_select.inc"') == 1
    assert text.index('#include "gf2_join_select.inc"') < text.index("}  // namespace")


def test_the_helpers_on_the_cpu(tmp_path):
    body = tmp_path / "join_select_body.inc"
    body.write_text(kt.extract_all(WORDS, SHARED) + "\n" + kt.extract_all(SELECT, HELPERS))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    exe = tmp_path / "join_select_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "join_select_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ranges = sum(1 for n in WIDTHS for wc0 in range(n + 1) for wc1 in range(wc0, n + 1))
    assert "%d ranges ok" % (3 * ranges) in run.stdout, run.stdout
    per_range = {n: 4 * (2 if n > 64 else 1) for n in WIDTHS}           # lanes x access widths
    pair_weights = sum(per_range[n] for n in WIDTHS for wc0 in range(n + 1) for wc1 in range(wc0, n + 1))
    assert "%d pair weights ok" % (3 * pair_weights) in run.stdout, run.stdout
    windows = sum((w + 3) * (w + 4) // 2 for n in WIDTHS for wc0 in range(n + 1) for w in range(n - wc0 + 1))
    assert int(re.search(r"(\d+) windows ok", run.stdout).group(1)) == 3 * windows, run.stdout
