"""The word-level helpers of the Hamming-distance search (m4ri-rust_amd/csrc/near/gf2_near.hip, near_plan.h) run on the CPU under the
host compiler's address and undefined-behaviour sanitizers (tests/near_emu.cpp), as tests/test_join_select_helpers_cpu.py does it for
the weight-filtered join: the shipped text, cut out with tests/kernel_text.py, in a program of its own; near_plan.h is plain host
arithmetic and is included as it is.

  near_first_word / near_end_word / gf2_word_mask (csrc/gf2_dev_words.h): the words and the bits of a range, over every range of ncols in {1, 63, 64, 65, 130}
  and a sample of those of 1100 columns; the masked popcounts sum to a bit-by-bit count.
  near_row_weight (the wide kernels) on rows in heap blocks of exactly the row's words; near_tile_row and near_weight (the register
  kernels) for W = 1, 2, 4, 8, 16 on every range that W words hold.
  near_in_window: every window 0 <= wlo <= whi <= width + 2 of every range, and whi = 2^31 - 1.
  near_pack_key / near_chunk_key / near_wide_key / near_key_dist / near_key_index: the order of the keys is that of (weight, row).
  near_excluded / near_tile_class against a loop over the pairs of a tile.
  near_chunk_begin / near_chunk_end / near_cell past 2^32, and near_plan over a table of shapes: the chunks cover B exactly.

No device is needed."""
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
NEAR = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "near")
KERNEL, PLAN = os.path.join(NEAR, "gf2_near.hip"), os.path.join(NEAR, "near_plan.h")
WORDS = os.path.join(os.path.dirname(NEAR), "gf2_dev_words.h")
HELPERS = ["kNearNoKey", "kNearNoKey64", "near_in_window", "near_excluded", "near_tile_class", "near_pack_key", "near_chunk_key",
           "near_wide_key", "near_key_dist", "near_key_index", "near_weight", "near_row_weight", "near_tile_row"]
WIDTHS = (1, 63, 64, 65, 130)


def test_the_new_kernels_use_no_atomics_and_no_assembly():
    shipped = kt.mask(open(KERNEL).read())
    assert "atomic" not in shipped and "asm" not in shipped
    assert kt.global_kernels(KERNEL) == ["gf2_near_kernel", "gf2_near_wide_kernel", "gf2_near_scan_kernel", "gf2_near_fold_kernel"]
    # the kernels weigh, test and rank a pair through the helpers alone
    assert shipped.count("__popcll(") == 2                       # near_weight and near_row_weight
    assert shipped.count("gf2_word_mask(") == 3                  # the masks of a range come from the shared helper: A, the tile, the wide rows
    assert shipped.count("near_in_window(") == 3 and shipped.count("near_excluded(") == 3 and shipped.count("near_pack_key(") == 2
    host = kt.mask(open(os.path.join(NEAR, "near_host.cpp")).read())
    assert "hipMalloc" not in host and "Synchronize" not in host
    plan = kt.mask(open(PLAN).read())
    assert "hip" not in plan.lower().replace("chip", "")         # plain host arithmetic


def test_the_helpers_on_the_cpu(tmp_path):
    body = tmp_path / "near_body.inc"
    body.write_text(kt.extract(WORDS, "gf2_word_mask") + "\n" + kt.extract_all(KERNEL, HELPERS))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    exe = tmp_path / "near_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", NEAR,
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "near_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    sample = len(range(0, 1101, 37))
    ranges = sum(1 for n in WIDTHS for wc0 in range(n + 1) for wc1 in range(wc0, n + 1)) + sample * (sample + 1) // 2
    assert "%d ranges ok" % (3 * ranges) in run.stdout, run.stdout
    windows = sum((w + 3) * (w + 4) // 2 for n in WIDTHS for wc0 in range(n + 1) for w in range(n - wc0 + 1))
    assert int(re.search(r"(\d+) windows ok", run.stdout).group(1)) == 3 * windows, run.stdout
    kernels = lambda words: sum(1 for W in (1, 2, 4, 8, 16) if words <= W)  # noqa: E731
    words = lambda wc0, wc1: (wc1 - 1) // 64 - wc0 // 64 + 1 if wc0 < wc1 else 0  # noqa: E731
    tiles = sum(kernels(words(wc0, wc1)) for n in WIDTHS for wc0 in range(n + 1) for wc1 in range(wc0, n + 1))
    tiles += sum(kernels(words(wc0, wc1)) for wc0 in range(0, 1101, 37) for wc1 in range(wc0, 1101, 37))
    assert "%d tile weights ok" % (3 * tiles) in run.stdout, run.stdout
    assert "%d keys ok" % (7 * 4 * 3 * 12) in run.stdout and "%d plans ok" % (10 * 11 * 7) in run.stdout, run.stdout
    assert "%d classes ok" % (4 * 3 * sum(15 - t0 for t0 in range(14))) in run.stdout, run.stdout
