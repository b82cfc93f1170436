"""The pair, start and head kernels and the index arithmetic of the scatter of the wide join
(m4ri-rust_amd/csrc/join_rows/gf2_join_rows.hip) run on the CPU under the host compiler's address and undefined-behaviour sanitizers
(tests/join_rows_emu.cpp), as tests/test_unique_kernels_cpu.py does it for the row sort: the shipped text, cut out with
tests/kernel_text.py, in a program of its own with its own main; join_rows_plan.h is plain arithmetic and is included as it is.

  the program's own checks: every window of the pair kernel, the chain of windows against one stable sort, the starts and heads of
  scattered classes, and output t -> (row of A, rank) by bisection of the offsets, then the chunk's first row and stretch: offsets
  with runs of zero multiplicities, a single row that owns more than a chunk of outputs, totals past 2^32.
  against the yardstick: on pools of tests/test_find_reference.py the program is given rep, idx and mult (tests/find_ref.py) and
  must print the order and head of join_rows_ref.group_rows and the ia, ib and count of join_rows_ref.join_rows, at several capacities.

The sum, scan, offset and scatter kernels cross lanes (shuffles, LDS) and are not emulated; tests/test_gpu_join_rows.py runs them.  No
device is needed."""
import os
import subprocess

import numpy as np
import pytest

import find_ref as fr
import join_rows_ref as jr
import kernel_text as kt
from test_find_reference import pools

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc")
MODULE = os.path.join(CSRC, "join_rows")
KERNEL, PLAN, HOST = (os.path.join(MODULE, f) for f in ("gf2_join_rows.hip", "join_rows_plan.h", "join_rows_host.cpp"))
KERNELS = ["gf2_join_rows_pairs_kernel", "gf2_join_rows_starts_kernel", "gf2_join_rows_heads_kernel", "gf2_join_rows_sums_kernel",
           "gf2_join_rows_scan_kernel", "gf2_join_rows_offsets_kernel", "gf2_join_rows_scatter_kernel"]


def test_the_new_kernels_use_no_atomics_and_the_host_one_slot():
    shipped = kt.mask(open(KERNEL).read())
    assert "atomic" not in shipped and "asm" not in shipped
    assert kt.global_kernels(KERNEL) == KERNELS
    assert shipped.count("template <int LANES>") == 3             # the scatter and its two row helpers: 1, 2, 8 or 64 lanes per row
    # the index arithmetic has one copy: the kernel calls what the CPU program runs
    assert shipped.count("join_rows_chunk_outputs(") == 1 and shipped.count("join_rows_chunk_rows(") == 2
    assert shipped.count("join_rows_output_row(") == 2 and shipped.count("join_rows_find_row(") == 3
    host = kt.mask(open(HOST).read())
    assert "hipMalloc" not in host and "Synchronize" not in host
    assert host.count("GF2_SLOT_JOIN_ROWS") == 2 and host.count("gf2_enqueue_mu") == 2 and "GF2_SLOT_FIND" not in host
    assert host.count("gf2k_find_rows(") == 2                       # A in B, and B in B inside the grouping: the table is built twice
    plan = kt.mask(open(PLAN).read())
    assert "hip" not in plan.lower().replace("m4ri_hip", "")       # plain arithmetic


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("join_rows_emu")
    body = tmp / "join_rows_body.inc"
    body.write_text(kt.extract_all(KERNEL, ["join_rows_chunk_rows", "join_rows_output_row", "gf2_join_rows_pairs_kernel",
                                            "gf2_join_rows_starts_kernel", "gf2_join_rows_heads_kernel"]))
    text = body.read_text()
    for word in ("atomic", "__shfl", "__ballot", "__shared__", "__syncthreads"):   # nothing that one CPU thread after the other cannot run
        assert word not in text, word
    exe = tmp / "join_rows_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", MODULE,
                           "-I", HERE, '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "join_rows_emu.cpp")])
    return exe


def test_the_kernels_and_the_index_arithmetic_on_the_cpu(emu):
    run = subprocess.run([str(emu)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    windows = sum(1 if bits <= 30 else 2 for bits in range(1, 32))
    assert "%d pair cases ok" % (2 * windows + 7) in run.stdout, run.stdout
    assert "24 start cases ok" in run.stdout and " outputs ok" in run.stdout, run.stdout
    assert int(run.stdout.split(" outputs ok")[0].split()[-1]) > 50000, run.stdout    # the program's own walk: six capacities past 7000 outputs


@pytest.mark.parametrize("case", [(200, 0, 0), (200, 5, 35), (200, 37, 82), (200, 0, 200), (704, 3, 700)], ids=lambda c: "%d-c%d-%d" % c)
def test_the_chain_against_the_yardstick(emu, tmp_path, case):
    ncols, c0, c1 = case
    for na, nb in ((1, 1), (40, 17), (300, 700), (2100, 2500)):
        if c0 == c1 and na > 300:
            continue                                                # every row meets every row: 210000 pairs are enough
        a, b = pools(ncols, c0, c1, na, nb, 41 + na)
        if (na, nb) == (40, 17):
            a, b = b[:17], b[:17]                                   # A == B
            na = 17
        rep, found = fr.find_rows(b, b, c0, c1).idx, fr.find_rows(a, b, c0, c1)
        want_order, want_head = jr.group_rows(b, c0, c1)
        full = jr.join_rows(a, b, ncols, c0, c1)
        for cap in sorted({1, full.count - 1, full.count, full.count + 5, 2048, 2049} - {0, -1}):
            path = tmp_path / "case.txt"
            path.write_text("%d %d %d\n%s\n%s\n%s\n" % (na, nb, cap, " ".join(map(str, rep)), " ".join(map(str, found.idx)),
                                                       " ".join(map(str, found.mult))))
            run = subprocess.run([str(emu), str(path)], capture_output=True, text=True)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
            out = {ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in run.stdout.splitlines()}
            assert np.array_equal(out["order"], want_order) and np.array_equal(out["head"], want_head), (case, na, nb)
            assert int(out["count"][0]) == full.count, (case, na, nb)
            n = min(cap, full.count)
            assert np.array_equal(out["ia"], full.ia[:n]) and np.array_equal(out["ib"], full.ib[:n]), (case, na, nb, cap)
        if c0 == c1:
            assert full.count == na * nb
        elif na > 2000:
            assert full.count > 2048 and (found.mult == 0).any()   # several chunks, and rows of A without a partner
