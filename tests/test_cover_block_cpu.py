"""The block reader and decoder of the covering-code kernels (cover_syn_bit / cover_block in m4ri-rust_amd/csrc/cover/gf2_cover.hip) and
the host routines gf2_cover_code_named / gf2_cover_leaders (cover_host.cpp) run on the CPU under the host compiler's address and
undefined-behaviour sanitizers (tests/cover_block_emu.cpp): the shipped text, cut out with tests/kernel_text.py, compiled into a
stand-alone program.  Every block offset 0 .. 127 against codes of n = 1, 7, 13, 23, 31 and 32 -- identity, drop and table codes -- on
rows whose heap block ends with the last word of the block, and again on a block that holds only the words with a bit of the block; the
tables are heap blocks of exactly 2^r words, and a code without a table gets neither table nor check rows.  Messages, weights, leaders
and radii must equal tests/cover_ref.py; a read of a word that holds no bit of the block is a sanitizer report, which a GPU test could
show only by faulting.  No device is needed."""
import os
import subprocess

import numpy as np

import cover_ref as cr
import gf2util as g
import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc")
KERNEL = os.path.join(CSRC, "cover", "gf2_cover.hip")
HOST = os.path.join(CSRC, "cover", "cover_host.cpp")
REPS, WORDS = 4, 3


def codes():
    wide = cr.Code(32, 22, tuple((int(x) & cr.mask(22)) | 1 << (22 + t) for t, x in enumerate(g.splitmix64(7, np.arange(10)))))
    return [cr.identity(1), cr.drop(1), cr.hamming(3), cr.golay23(), cr.hamming(5), cr.identity(32), cr.drop(32), cr.repetition(13), wide]


def test_the_block_helper_reads_only_the_words_of_the_block(tmp_path):
    body = tmp_path / "block_body.inc"
    body.write_text(kt.extract_all(KERNEL, ["CoverBlock", "cover_syn_bit", "cover_block"]))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads", "threadIdx"):   # nothing a single CPU thread cannot run
        assert word not in text, word
    assert "__host__ __device__" in text
    # the kernel reads and decodes a block through this function alone
    shipped = kt.mask(open(KERNEL).read())
    assert shipped.count("cover_block(") == 2 and shipped.count("__global__") == 1     # its definition and the one call of the one kernel
    host = tmp_path / "host_body.inc"
    host.write_text(kt.extract_all(HOST, ["kGolayG", "top_bit", "gf2_cover_code_named", "gf2_cover_leaders"]))
    exe = tmp_path / "cover_block_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, '-DKERNEL_BODY="%s"' % body, '-DHOST_BODY="%s"' % host, "-o", str(exe),
                           os.path.join(HERE, "cover_block_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    cs = codes()
    assert {c.n for c in cs} == {1, 7, 13, 23, 31, 32}
    assert lines[-1] == "%d blocks ok" % (len(cs) * 128 * REPS)
    words = g.splitmix64(2026, np.arange(REPS * WORDS)).reshape(REPS, WORDS)
    got_codes = [ln.split() for ln in lines if ln.startswith("code ")]
    got_leaders = np.array([ln.split()[1:] for ln in lines if ln.startswith("L ")], dtype=np.int64)
    got_blocks = np.array([ln.split()[1:] for ln in lines if ln.startswith("B ")], dtype=np.int64)
    assert len(got_codes) == len(cs) and got_blocks.shape == (len(cs) * 128 * REPS, 5)
    for ci, code in enumerate(cs):
        table, radius = cr.leaders(code)
        assert got_codes[ci] == ["code", str(ci), str(code.n), str(code.k), "radius", str(radius)]
        mine = got_leaders[got_leaders[:, 0] == ci]
        if cr.has_table(code):
            assert np.array_equal(mine[:, 1], np.arange(len(table))) and np.array_equal(mine[:, 2], table), ci
        else:
            assert len(mine) == 0
        for o in range(128):
            D, dist = cr.reduce(words, o, [code])
            rows = got_blocks[(got_blocks[:, 0] == ci) & (got_blocks[:, 1] == o)]
            assert np.array_equal(rows[:, 2], np.arange(REPS))
            assert np.array_equal(rows[:, 3], D[:, 0] if code.k else np.zeros(REPS)) and np.array_equal(rows[:, 4], dist), (ci, o)
