"""The rekey kernel and the row compare of the row sort (m4ri-rust_amd/csrc/unique/gf2_unique.hip) run on the CPU under the host
compiler's address and undefined-behaviour sanitizers (tests/unique_emu.cpp), as tests/test_dev_words_cpu.py does it for the shared
helpers: the shipped text, cut out with tests/kernel_text.py, in a program of its own; unique_plan.h is plain host arithmetic and is
included as it is.

  gf2_unique_rekey_kernel, thread by thread: every window of every range [c0, c1) of ncols in {1, 63, 64, 65, 130}, on a row whose heap
  block holds only the words with a bit of the window; every key equals the bit-by-bit definition, and the windows cover the range once.
  unique_rows_differ: every such range on rows whose heap blocks hold only the words with a bit of the range; every compare equals the
  bit-by-bit definition -- bits outside the range never count, every column of the range does -- and nothing is read behind the
  first difference.
A read of a word that holds no bit of the range is a sanitizer report, which a GPU test could show only by faulting.

The other kernels of the file cross lanes (shuffles, LDS) and are not emulated; tests/test_gpu_unique.py runs them.  No device is needed."""
import os
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc")
UNIQUE = os.path.join(CSRC, "unique")
KERNEL, PLAN, HOST = os.path.join(UNIQUE, "gf2_unique.hip"), os.path.join(UNIQUE, "unique_plan.h"), os.path.join(UNIQUE, "unique_host.cpp")
WORDS = os.path.join(CSRC, "gf2_dev_words.h")
WIDTHS = (1, 63, 64, 65, 130)


def test_the_new_kernels_use_no_atomics_and_no_assembly():
    shipped = kt.mask(open(KERNEL).read())
    assert "atomic" not in shipped and "asm" not in shipped
    assert kt.global_kernels(KERNEL) == ["gf2_unique_rekey_kernel", "gf2_unique_heads_kernel", "gf2_unique_carry_kernel",
                                         "gf2_unique_fill_kernel", "gf2_unique_rep_kernel"]
    assert "template" not in shipped                               # one instance of each: the census needs no table of shapes
    # a row is read through the shared helpers alone: the key of a window, the mask of a word of the range
    assert shipped.count("gf2_row_key(") == 1 and shipped.count("gf2_word_mask(") == 1 and shipped.count("unique_rows_differ(") == 2
    assert "uint4" not in shipped                                  # no 16-byte access
    host = kt.mask(open(HOST).read())
    assert "hipMalloc" not in host and "Synchronize" not in host
    assert host.count("GF2_SLOT_UNIQUE") == 2 and host.count("gf2_enqueue_mu") == 2      # both entries, under the lock
    plan = kt.mask(open(PLAN).read())
    assert "hip" not in plan.lower()                               # plain host arithmetic


def test_the_rekey_kernel_and_the_compare_on_the_cpu(tmp_path):
    body = tmp_path / "unique_body.inc"
    body.write_text(kt.extract_all(WORDS, ["Gf2KeyWindow", "gf2_key_window", "gf2_row_key", "gf2_word_mask"]) + "\n" +
                    kt.extract_all(KERNEL, ["unique_rows_differ", "gf2_unique_rekey_kernel"]))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads"):   # nothing that one CPU thread after the other cannot run
        assert word not in text, word
    exe = tmp_path / "unique_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", UNIQUE,
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "unique_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ranges = sum(1 for n in WIDTHS for c0 in range(n + 1) for c1 in range(c0, n + 1))
    columns = sum(c1 - c0 for n in WIDTHS for c0 in range(n + 1) for c1 in range(c0, n + 1))
    assert "%d keys ok" % (3 * ranges + 2) in run.stdout, run.stdout
    assert "%d compares ok" % (ranges + columns) in run.stdout, run.stdout
