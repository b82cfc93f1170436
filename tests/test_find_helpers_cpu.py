"""The hash, the compare, the slot sequence and the lane forms of insert and probe of the row lookup
(m4ri-rust_amd/csrc/find/gf2_find.hip, find_plan.h) run on the CPU under the host compiler's address and undefined-behaviour sanitizers
(tests/find_emu.cpp), as tests/test_unique_kernels_cpu.py does it for the row sort: the shipped text, cut out with tests/kernel_text.py,
in a stand-alone program of its own; find_plan.h is plain arithmetic and is included as it is.

  find_row_hash, find_rows_equal: every range [c0, c1) of ncols in {1, 63, 64, 65, 130} on rows whose heap blocks hold only the words
  with a bit of the range: bits outside the range never count, every column of the range does, and the compare reads nothing behind the
  first difference.
  find_first_slot, find_next_slot, find_entry: the sequence visits every slot once and wraps; 2^32 slots; entries of one tag order by row.
  find_insert, find_probe: a serial build and lookup with tables forced small (4, 8 and 64 slots, slots - 1 distinct rows plus
  duplicates -- loads the device entry never reaches): wrap-around, a miss that ends at the one empty slot, the lowest row of a class
  for three arrival orders.  The program prints pools and results; they are compared with tests/find_ref.py here.
A read of a word that holds no bit of the range, or of a slot outside the table, is a sanitizer report.

The wave forms and the kernels cross lanes (shuffles, ballots, LDS) and are not emulated; tests/test_gpu_find.py runs them.  No device
is needed."""
import os
import subprocess

import numpy as np

import find_ref as fr
import kernel_text as kt

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc")
FIND = os.path.join(CSRC, "find")
KERNEL, PLAN, HOST = os.path.join(FIND, "gf2_find.hip"), os.path.join(FIND, "find_plan.h"), os.path.join(FIND, "find_host.cpp")
WORDS = os.path.join(CSRC, "gf2_dev_words.h")
WIDTHS = (1, 63, 64, 65, 130)
KERNELS = ["gf2_find_fill_kernel", "gf2_find_build_kernel", "gf2_find_lookup_kernel"]


def test_the_layout_of_the_module():
    shipped = kt.mask(open(KERNEL).read())
    assert kt.global_kernels(KERNEL) == KERNELS
    assert "asm" not in shipped and "uint4" not in shipped                      # no assembly, no 16-byte access
    for word in ("while", "goto", "__builtin_amdgcn_s_sleep", "clock"):         # no spin: every loop is a bounded for
        assert word not in shipped, word
    assert shipped.count("step < slots") == 4                                    # the four probe loops carry the bound
    # a row is read through the shared mask alone, in the two hashes and the two compares
    assert shipped.count("gf2_word_mask(") == 4
    # the atomics: one compare-and-swap, one minimum and one count per form of the build, the hits of a workgroup and *count
    assert shipped.count("atomicCAS(") == 2 and shipped.count("atomicMin(") == 2 and shipped.count("atomicAdd(") == 5
    assert "atomicExch" not in shipped and "float" not in shipped
    host = kt.mask(open(HOST).read())
    assert "hipMalloc" not in host and "Synchronize" not in host
    assert host.count("GF2_SLOT_FIND") == 1 and host.count("gf2_enqueue_mu") == 1
    assert "GF2_SLOT_FIND = 18" in open(os.path.join(CSRC, "api_internal.h")).read()
    plan = kt.mask(open(PLAN).read())
    assert "hip" not in plan.lower() and "__device__" not in plan              # plain arithmetic for host and device
    mk = open(os.path.join(CSRC, "sources.mk")).read()
    for name in ("find/gf2_find.hip", "find/find_host.cpp", "find/find_plan.h", "find/gf2_find.h ", "m4ri_hip_find.h"):
        assert mk.count(name) == 1, name


def parse(stdout):
    cases, cur = [], None
    for ln in stdout.splitlines():
        tag, _, rest = ln.partition(" ")
        if tag == "CASE":
            cur = dict(zip(("slots", "ncols", "c0", "c1", "na", "nb"), map(int, rest.split())), A=[], B=[])
            cases.append(cur)
        elif tag in ("A", "B"):
            cur[tag].append([int(x, 16) for x in rest.split()])
        elif tag in ("IDX", "MULT"):
            cur[tag] = np.array([int(x) for x in rest.split()], dtype=np.int32)
    return cases


def test_hash_compare_slots_and_small_tables_on_the_cpu(tmp_path):
    body = tmp_path / "find_body.inc"
    body.write_text(kt.extract_all(WORDS, ["gf2_word_mask"]) + "\n" +
                    kt.extract_all(KERNEL, ["find_row_hash", "find_rows_equal", "find_insert", "find_probe"]))
    text = body.read_text()
    for word in ("__shfl", "__ballot", "__any", "__shared__", "__syncthreads", "threadIdx"):   # nothing that one CPU thread after the other cannot run
        assert word not in text, word
    exe = tmp_path / "find_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", FIND,
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "find_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ranges = sum(1 for n in WIDTHS for c0 in range(n + 1) for c1 in range(c0, n + 1))
    columns = sum(c1 - c0 for n in WIDTHS for c0 in range(n + 1) for c1 in range(c0, n + 1))
    assert "%d hashes and compares ok" % (ranges + columns) in run.stdout, run.stdout[-500:]
    assert "%d slot sequences ok" % (2 + 4 + 8 + 64 + 3) in run.stdout, run.stdout[-500:]
    assert "15 tables ok" in run.stdout, run.stdout[-500:]
    cases = parse(run.stdout)
    assert [c["slots"] for c in cases] == [4] * 5 + [8] * 5 + [64] * 5
    for c in cases:
        a, b = np.array(c["A"], dtype=np.uint64), np.array(c["B"], dtype=np.uint64)
        assert len(a) == c["na"] == 2 * c["slots"] + 3 and len(b) == c["nb"]
        want = fr.find_rows(a, b, c["c0"], c["c1"])
        assert np.array_equal(c["IDX"], want.idx) and np.array_equal(c["MULT"], want.mult), c
        width = c["c1"] - c["c0"]
        if width >= 8:
            assert c["nb"] == c["slots"] - 1 + c["slots"] // 2 + 1 and len(set(want.idx[want.idx >= 0])) > 1
            assert 0 < want.count < c["na"] and want.mult.max() > 1             # hits, misses and classes of several members
            assert len(np.unique(b[want.idx[want.idx >= 0]], axis=0)) <= c["slots"] - 1
        elif width == 0:
            assert not want.idx.any() and (want.mult == c["nb"]).all()
