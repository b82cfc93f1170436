"""The kernels of m4ri-rust_amd/csrc/gather on the CPU side of the suite (no device is needed).

tests/test_kernels_cpu.py::test_every_kernel_is_classified keeps a closed list of the kernels of csrc/*.hip; the same rule is applied
here to csrc/gather/*.hip with a list of its own: every __global__ kernel is either run thread by thread under the host compiler's
address and undefined-behaviour sanitizers (EMULATED) or named with the words of the scope rule that keep it off the CPU
(NOT_EMULATED: cross-lane, LDS, barriers, atomics, inline assembly).

The row-gather kernel is a word-level kernel: its shipped text, cut out with tests/kernel_text.py, runs in tests/gather_emu.cpp behind
tests/kernel_emu.h, a stand-alone program with its own main.  Buffers end with the last word of the operand's last row and the index
array with its last int, so a load or store of a word that holds no bit of the operand is a sanitizer report, and the launcher's choice
of 16-byte pieces is judged by the alignment check over every parity of both row strides and both bases."""
import glob
import os
import re
import subprocess
import sys

import kernel_text

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GATHER = os.path.join(ROOT, "m4ri-rust_amd", "csrc", "gather")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# what the program needs, in order: helper, kernel, launcher
# the shared helpers of csrc/gf2_dev_words.h that they call: their text counts as the kernel's and the launcher's
SHARED = ["gf2_lo_hi", "gf2_rows_aligned16"]
PIECES = ["gf2_gather_rows_kernel", "gf2k_gather_rows"]
# widths 6 x (D rows, S rows) 4 x (ld of D 3 x ld of S 3 x base of D 2 x base of S 2) x plain / accumulate x two index patterns
EMULATED = {"gf2_gather_rows_kernel": ("gf2_gather_rows_kernel", 6 * 4 * 36 * 2 * 2)}
NOT_EMULATED = {"gf2_gather_cols_kernel": "LDS, barriers, cross-lane"}
RULE_WORDS = {"cross-lane", "LDS", "barriers", "atomics", "inline assembly"}
# how each rule word shows in a kernel's text (helpers it calls included)
SIGNS = {
    "cross-lane": r"__shfl|__ballot|__any\b|__all\b|ds_swizzle|ds_bpermute|ds_permute|readlane|readfirstlane|permlane|__builtin_amdgcn_mov_dpp",
    "LDS": r"__shared__",
    "barriers": r"__syncthreads|s_barrier",
    "atomics": r"\batomic\w+\s*\(|__atomic_|__hip_atomic",
    "inline assembly": r"\basm\b",
}


def pieces_text():
    words = os.path.join(ROOT, "m4ri-rust_amd", "csrc", "gf2_dev_words.h")
    return kernel_text.extract_all(words, SHARED) + "\n" + kernel_text.extract_all(os.path.join(GATHER, "gf2_gather.hip"), PIECES)


def sources():
    return sorted(glob.glob(os.path.join(GATHER, "*.hip")) + glob.glob(os.path.join(GATHER, "*.inc")))


def test_every_gather_kernel_is_classified():
    srcs = sources()
    assert [os.path.basename(s) for s in srcs] == ["gf2_gather.hip"]
    names = [k for path in srcs for k in kernel_text.global_kernels(path)]
    assert len(names) == len(set(names)) == 2, names
    assert not set(EMULATED) & set(NOT_EMULATED)
    missing = set(names) - set(EMULATED) - set(NOT_EMULATED)
    assert not missing, "new kernels: give each a driver in tests/gather_emu.cpp or a reason in NOT_EMULATED: %s" % sorted(missing)
    gone = (set(EMULATED) | set(NOT_EMULATED)) - set(names)
    assert not gone, "listed here, but no longer in csrc/gather: %s" % sorted(gone)
    for name, reason in NOT_EMULATED.items():
        for word in reason.split(", "):
            assert word in RULE_WORDS, (name, word)
    assert set(EMULATED) <= set(PIECES), "emulated, but not cut out of its file"
    # no name twice across the library: the frozen list of tests/test_kernels_cpu.py and this one describe one set of kernels
    csrc = os.path.dirname(GATHER)
    older = [k for p in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.inc"))) for k in kernel_text.global_kernels(p)]
    assert not set(older) & set(names)


def test_the_reasons_match_the_text():
    """an emulated kernel shows none of the signs; a kernel that is not emulated shows each sign its reason names"""
    path = sources()[0]
    whole = kernel_text.mask(open(path).read())
    assert not re.search(SIGNS["inline assembly"], whole) and not re.search(SIGNS["atomics"], whole)   # the file uses neither at all
    for name in EMULATED:
        text = kernel_text.mask(pieces_text())
        for word, sign in SIGNS.items():
            assert not re.search(sign, text), (name, word)
    for name, reason in NOT_EMULATED.items():
        text = kernel_text.mask(kernel_text.extract(path, name) + kernel_text.extract(path, "gather_transpose64"))
        for word in reason.split(", "):
            assert re.search(SIGNS[word], text), (name, word)


def test_row_kernel_touches_only_words_of_its_operands(tmp_path):
    body = tmp_path / "gather_body.inc"
    body.write_text(pieces_text())
    exe = tmp_path / "gather_emu"
    build = subprocess.run(["g++"] + FLAGS + ['-DKERNEL_BODY="%s"' % body, "-I", HERE, "-o", str(exe), os.path.join(HERE, "gather_emu.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-6000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    assert "all ok" in run.stdout, run.stdout
    counts = {label: int(n) for label, n in re.findall(r"^(.+): (\d+) cases ok$", run.stdout, re.M)}
    for kernel, (label, n) in EMULATED.items():
        assert counts.get(label) == n, (kernel, counts)


def test_hazard_audit_of_the_gather_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import asm_hazards
    finally:
        sys.path.pop(0)
    findings, stats = asm_hazards.audit(sources=[s for s in sources() if s.endswith(".hip")])
    assert stats["functions"] >= 2 and stats["instructions"] > 100, stats
    assert stats["asm_instructions"] == 0, stats   # builtins and plain C++ only
    assert not findings, findings
