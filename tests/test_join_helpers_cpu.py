"""The word-level helpers of the join kernels (m4ri-rust_amd/csrc/join/gf2_join.hip) run on the CPU under the host compiler's address
and undefined-behaviour sanitizers (tests/join_emu.cpp), as tests/test_lf2_key_cpu.py does it for LF2: the shipped text, cut out with
tests/kernel_text.py.

  join_lower_bound / join_upper_bound: the first position of [lo, hi) whose key is not below / is above a value, on sorted keys in a
  heap block that holds the positions [lo, hi) alone: the first and the last element, a key that is absent, below all or above all,
  one giant class.
  join_find_position: the position that an output of a run belongs to, on sums with empty positions, one giant position and 64-bit
  totals.
  join_word_weight: the ones of a word in a column range, over every [wc0, wc1) of ncols in {1, 63, 64, 65, 130}, against a
  bit-by-bit count.

No device is needed."""
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "join", "gf2_join.hip")
HELPERS = ["join_lower_bound", "join_upper_bound", "join_find_position", "join_word_weight"]
WIDTHS = (1, 63, 64, 65, 130)


def test_the_helpers_read_only_what_they_may(tmp_path):
    body = tmp_path / "join_body.inc"
    body.write_text(kt.extract_all(KERNEL, HELPERS))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    # the kernels find their partners, their positions and their weights through these helpers alone
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("join_lower_bound(") == 4 and shipped.count("join_upper_bound(") == 4      # the definition, the span, LDS, global
    assert shipped.count("join_find_position(") == 2 and shipped.count("join_word_weight(") == 4
    assert shipped.count("__popcll(") == 1 and "atomic" not in shipped and "asm" not in shipped
    exe = tmp_path / "join_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "join_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ranges = sum(1 for n in WIDTHS for wc0 in range(n + 1) for wc1 in range(wc0, n + 1))
    assert "%d weights ok" % (3 * ranges) in run.stdout, run.stdout
    bounds = re.search(r"(\d+) bounds ok", run.stdout)
    positions = re.search(r"(\d+) positions ok", run.stdout)
    assert bounds and int(bounds.group(1)) >= 4000 and positions and int(positions.group(1)) >= 1000, run.stdout
