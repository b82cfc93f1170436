"""The routines of the order of the subset sums (m4ri-rust_amd/csrc/sums/sums_plan.h: binomial, rank, unrank, advance by a stride) run
on the CPU under the host compiler's address and undefined-behaviour sanitizers (tests/sums_emu.cpp), as
tests/test_join_helpers_cpu.py does it for the join: the shipped text, cut out with tests/kernel_text.py.

  sums_binomial: against 128-bit arithmetic up to the largest c of every level (sums_max_c), which is the largest.
  sums_advance: for every p in 1 .. 4, n <= 14, every start rank and the strides 1, 2, 3, 64, 65, 1000, against single steps, against
  sums_unrank of the rank further on, and its carry flag against what changed.
  sums_unrank: at ranks around 2^31, 2^32 and 2^62.

The word weight of the kernel is a shared helper (gf2_word_weight of csrc/gf2_dev_words.h): tests/test_dev_words_cpu.py runs its
cases; here is what the kernel file may and may not do with it.

No device is needed."""
import math
import os
import re
import subprocess

import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "sums")
PLAN, KERNEL = os.path.join(CSRC, "sums_plan.h"), os.path.join(CSRC, "gf2_sums.hip")
ORDER = ["kSumsMaxP", "kSumsNone", "sums_max_c", "sums_binomial", "sums_rank", "sums_unrank", "sums_advance"]
STRIDES = (1, 2, 3, 64, 65, 1000)


def test_the_shipped_order_routines_and_the_word_weight(tmp_path):
    body = tmp_path / "sums_body.inc"
    body.write_text(kt.extract_all(PLAN, ORDER))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    # the kernels rank, unrank, advance and weigh through these routines alone, and the host entries are wrappers over the same text
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("sums_unrank(") == 2 and shipped.count("sums_advance(") == 1 and shipped.count("gf2_word_weight(") == 3
    assert shipped.count("__popcll(") == 0 and "atomic" not in shipped and "asm" not in shipped
    host = kt.mask(open(os.path.join(CSRC, "sums_host.cpp")).read())
    assert "sums_unrank(" in host and "sums_rank(" in host and "sums_count(" in host and "comb" not in host
    exe = tmp_path / "sums_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "sums_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    starts = sum(math.comb(n, p) for p in range(1, 5) for n in range(p, 15))
    assert "%d advances ok" % (len(STRIDES) * starts) in run.stdout, run.stdout
    binomials = re.search(r"(\d+) binomials ok", run.stdout)
    unranks = re.search(r"(\d+) unranks ok", run.stdout)
    assert binomials and int(binomials.group(1)) >= 4 * 2300 and unranks and int(unranks.group(1)) == 4 * (4 + 3 * 141), run.stdout
