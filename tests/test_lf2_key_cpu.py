"""The word-level helper that the LF2 kernels keep for themselves (m4ri-rust_amd/csrc/lf2/gf2_lf2.hip) run on the CPU under the host
compiler's address and undefined-behaviour sanitizers (tests/lf2_key_emu.cpp): the shipped text, cut out with tests/kernel_text.py.

  lf2_class_start: the first position of a class, from any of its members, on a block that ends with that member.

The key reader and the position of an output are shared helpers (gf2_row_key, gf2_find_position of csrc/gf2_dev_words.h):
tests/test_dev_words_cpu.py runs their cases; here is what the kernel file may and may not do with them.

No device is needed."""
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "lf2", "gf2_lf2.hip")
BKW = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "bkw", "gf2_bkw.hip")


def test_the_helpers_read_only_what_they_may(tmp_path):
    body = tmp_path / "key_body.inc"
    body.write_text(kt.extract_all(KERNEL, ["lf2_class_start"]))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    # the kernels read the key through the shared function alone, and their other lookups through the two helpers
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("gf2_row_key(") == 2              # the count and the scatter kernel of the sort
    assert shipped.count("lf2_class_start(") == 2 and shipped.count("gf2_find_position(") == 1
    assert "lf1_key" not in shipped and "lf2_key" not in shipped and "w.w0" not in shipped     # the window's words are named in the header alone
    exe = tmp_path / "lf2_key_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "lf2_key_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    starts = re.search(r"(\d+) class starts ok", run.stdout)
    assert starts and int(starts.group(1)) >= 400, run.stdout


def test_the_rule_is_the_rule_of_the_lf1_key():
    """LF1 and LF2 have one key reader: neither file defines one, both call the shared one"""
    for path in (KERNEL, BKW):
        text = open(path).read()
        for name in ("gf2_row_key", "gf2_key_window", "Gf2KeyWindow", "lf1_key", "lf2_key", "lf1_window", "lf2_window", "Lf1Window", "Lf2Window"):
            assert not kt._definitions(text, name), (path, name)
        shipped = kt.mask(text)
        assert '#include "../gf2_dev_words.h"' in text and shipped.count("gf2_row_key(") >= 2 and shipped.count("gf2_key_window(") >= 2
