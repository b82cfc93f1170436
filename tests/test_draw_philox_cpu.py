"""The shipped generator and per-word rules of the device draws (m4ri-rust_amd/csrc/draw/philox.h) on the CPU under the host compiler's
address and undefined-behaviour sanitizers (tests/draw_emu.cpp), on the pattern of tests/test_lf2_key_cpu.py.  The header is included
as it is shipped -- the kernels make every value through its functions --, and every line the program prints must be what the
yardstick of tests/draw_ref.py gives for the same input: Philox blocks (the published known answers among them), Bernoulli words at
thresholds with no plane, one call, all sixteen calls and all ones, at word indices on either side of 2^32 and up to 2^64 - 1, index
pairs, subset candidates and permutation keys.

No device is needed."""
import os
import subprocess

import draw_ref as dr

HERE = os.path.dirname(os.path.abspath(__file__))
DRAW = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "draw")


def test_the_kernels_make_their_values_through_the_header():
    """no second copy of a rule in the kernel file: it names no multiplier, no key increment and no tag, and calls the header's
    functions where it needs a value"""
    text = open(os.path.join(DRAW, "gf2_draw.hip")).read()
    for word in ("D2511F53", "CD9E8D57", "9E3779B9", "BB67AE85", "philox4x32_10(", "kDrawTag"):
        assert word.lower() not in text.lower(), word
    for call in ("draw_bernoulli_word(", "draw_index_pair(", "draw_subset_candidate(", "draw_perm_key("):
        assert call in text, call
    header = open(os.path.join(DRAW, "philox.h")).read()
    assert "asm" not in header and "__host__ __device__" in header


def test_the_shipped_functions_equal_the_yardstick(tmp_path):
    exe = tmp_path / "draw_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-Werror", "-I", DRAW, "-o", str(exe), os.path.join(HERE, "draw_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    seen = {}
    for line in run.stdout.splitlines():
        kind, rest = line.split(None, 1)
        args, got = ([int(v, 16) for v in part.split()] for part in rest.split("->"))
        seen[kind] = seen.get(kind, 0) + 1
        if kind == "K":
            want = [int(x[0]) for x in dr.philox(*args)]
        elif kind == "B":
            seed, widx, thr = args
            want = [int(dr.bernoulli_words(seed, [widx], thr)[0][0])]
            assert want == [int(dr.bernoulli_words_by_bits(seed, [widx], thr)[0])], line
        elif kind == "I":
            seed, p, n = args
            x = dr.block(seed, [p], 0, dr.TAG_INDICES)
            want = [int(dr.below(x[0], x[1], n)[0]), int(dr.below(x[2], x[3], n)[0])]
            assert all(0 <= v < n for v in want), line
        elif kind == "S":
            seed, at, a, n = args
            want = [int(dr.subset_candidates(seed, [at], a, n)[0])]
        elif kind == "P":
            seed, i = args
            want = [int(dr.block(seed, [i], 0, dr.TAG_PERMUTATION)[0][0]) & ((1 << 30) - 1)]
        else:
            assert kind == "C", line
            want = [dr.bernoulli_words(0, [0], args[0])[1]]
        assert got == want, (line, want)
    assert seen == {"K": 4, "B": 270, "I": 135, "S": 405, "P": 27, "C": 10}, seen
    answers = [ln.split("->")[1].split() for ln in run.stdout.splitlines()[:3]]
    assert answers == [["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"], ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"],
                       ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]]
