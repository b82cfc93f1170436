"""The word-level helpers that the join kernels keep for themselves (m4ri-rust_amd/csrc/join/gf2_join.hip) run on the CPU under the
host compiler's address and undefined-behaviour sanitizers (tests/join_emu.cpp), as tests/test_lf2_key_cpu.py does it for LF2: the
shipped text, cut out with tests/kernel_text.py.

  join_lower_bound / join_upper_bound: the first position of [lo, hi) whose key is not below / is above a value, on sorted keys in a
  heap block that holds the positions [lo, hi) alone: the first and the last element, a key that is absent, below all or above all,
  one giant class.

The position of an output and the weight of a column range are shared helpers (gf2_find_position, gf2_word_weight of
csrc/gf2_dev_words.h): tests/test_dev_words_cpu.py runs their cases; here is what the kernel file may and may not do with them.

No device is needed."""
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "join", "gf2_join.hip")
HELPERS = ["join_lower_bound", "join_upper_bound"]


def test_the_helpers_read_only_what_they_may(tmp_path):
    body = tmp_path / "join_body.inc"
    body.write_text(kt.extract_all(KERNEL, HELPERS))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    # the kernels find their partners, their positions and their weights through these helpers alone
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("join_lower_bound(") == 4 and shipped.count("join_upper_bound(") == 4      # the definition, the span, LDS, global
    assert shipped.count("gf2_find_position(") == 1 and shipped.count("gf2_word_weight(") == 3       # no definition here: the calls alone
    assert shipped.count("__popcll(") == 0 and "atomic" not in shipped and "asm" not in shipped      # the popcount is in the header alone
    exe = tmp_path / "join_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "join_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    bounds = re.search(r"(\d+) bounds ok", run.stdout)
    assert bounds and int(bounds.group(1)) >= 4000, run.stdout
