"""The word-level helpers of the LF2 kernels (m4ri-rust_amd/csrc/lf2/gf2_lf2.hip) run on the CPU under the host compiler's address and
undefined-behaviour sanitizers (tests/lf2_key_emu.cpp), as tests/test_bkw_key_cpu.py does it for LF1: the shipped text, cut out with
tests/kernel_text.py.

  lf2_window / lf2_key: every window [c0, c0 + b) with c0 + b <= ncols, b <= 30, for ncols in {1, 63, 64, 65, 128, 130}, on rows whose
  heap block ends with the last word of the row, and again on a block that holds only the words with a bit of the window.  Every key
  must equal the bit-by-bit definition; a read of a word that holds no bit of the window is a sanitizer report.
  lf2_class_start: the first position of a class, from any of its members, on a block that ends with that member.
  lf2_find_position: the position that an output of a run belongs to, on sums with empty positions, one giant position and 64-bit
  totals.

No device is needed."""
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "lf2", "gf2_lf2.hip")
BKW = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "bkw", "gf2_bkw.hip")
WIDTHS = (1, 63, 64, 65, 128, 130)


def test_the_helpers_read_only_what_they_may(tmp_path):
    body = tmp_path / "key_body.inc"
    body.write_text(kt.extract_all(KERNEL, ["Lf2Window", "lf2_window", "lf2_key", "lf2_class_start", "lf2_find_position"]))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    # the kernels read the key through this function alone, and their other lookups through the two helpers
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("lf2_key(") == 3              # its definition, the count and the scatter kernel of the sort
    assert shipped.count("lf2_class_start(") == 2 and shipped.count("lf2_find_position(") == 2
    assert "lf1_key" not in shipped and shipped.count("w.w0") == 3     # the window's words are named there and nowhere else
    exe = tmp_path / "lf2_key_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "lf2_key_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    windows = sum(1 for n in WIDTHS for c0 in range(n + 1) for b in range(31) if c0 + b <= n)
    assert "%d keys ok" % (3 * windows) in run.stdout, run.stdout
    starts = re.search(r"(\d+) class starts ok", run.stdout)
    positions = re.search(r"(\d+) positions ok", run.stdout)
    assert starts and int(starts.group(1)) >= 400 and positions and int(positions.group(1)) >= 1000, run.stdout


def test_the_rule_is_the_rule_of_the_lf1_key():
    """the two key readers differ in their names alone"""
    mine = kt.extract_all(KERNEL, ["Lf2Window", "lf2_window", "lf2_key"])
    theirs = kt.extract_all(BKW, ["Lf1Window", "lf1_window", "lf1_key"])
    assert mine.replace("Lf2", "Lf1").replace("lf2", "lf1") == theirs
