"""The key reader of the LF1 kernels (lf1_window / lf1_key in m4ri-rust_amd/csrc/bkw/gf2_bkw.hip) run on the CPU under the host
compiler's address and undefined-behaviour sanitizers (tests/bkw_key_emu.cpp): the shipped text, cut out with tests/kernel_text.py,
over every window [c0, c0 + b) with c0 + b <= ncols, b <= 30, for ncols in {1, 63, 64, 65, 128, 130}, on rows whose heap block ends with
the last word of the row, and again on a block that holds only the words with a bit of the window.  Every key must equal the
bit-by-bit definition; a read of a word that holds no bit of the window is a sanitizer report, which a GPU test could show only by
faulting.  No device is needed."""
import os
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "bkw", "gf2_bkw.hip")
WIDTHS = (1, 63, 64, 65, 128, 130)


def test_the_key_reads_only_the_words_of_the_window(tmp_path):
    body = tmp_path / "key_body.inc"
    body.write_text(kt.extract_all(KERNEL, ["Lf1Window", "lf1_window", "lf1_key"]))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    # the kernels read the key through this function alone
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("lf1_key(") == 3     # its definition, the class firsts, the survivor rule of count and scatter
    exe = tmp_path / "bkw_key_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "bkw_key_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    windows = sum(1 for n in WIDTHS for c0 in range(n + 1) for b in range(31) if c0 + b <= n)
    assert "%d keys ok" % (3 * windows) in run.stdout, run.stdout
