"""The kernels of m4ri-rust_amd/csrc/weight on the CPU side of the suite (no device is needed).

The classification rule of tests/test_kernels_cpu.py::test_every_kernel_is_classified and tests/test_gather_kernels_cpu.py, applied to
csrc/weight/*.hip with a list of its own: every __global__ kernel is either run thread by thread under the host compiler's address and
undefined-behaviour sanitizers (EMULATED) or named with the words of the scope rule that keep it off the CPU (NOT_EMULATED: cross-lane,
LDS, barriers, atomics, inline assembly).

The narrow row-weight kernel (one lane per row) is a word-level kernel: its shipped text, cut out with tests/kernel_text.py, runs in
tests/weight_emu.cpp behind tests/kernel_emu.h, a stand-alone program with its own main.  The operand ends with the last word of its
last row and `weights` with its last int, so a read of a pad word or of a word past the row width is a sanitizer report, and the
launcher's choice of 16-byte loads is judged by the alignment check over three row strides and both base parities."""
import glob
import os
import re
import subprocess
import sys

import kernel_text

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WEIGHT = os.path.join(ROOT, "m4ri-rust_amd", "csrc", "weight")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# what the program needs, in order: helpers, kernel, launcher
# the shared helpers of csrc/gf2_dev_words.h that they call: their text counts as the kernel's and the launcher's
SHARED = ["gf2_lo_hi", "gf2_rows_aligned16"]
PIECES = ["weight_row_partial", "gf2_weight_rows_narrow_kernel", "gf2k_weight_rows_narrow"]
# widths 9 x rows 4 x (ld 3 x base 2) x content 3
EMULATED = {"gf2_weight_rows_narrow_kernel": ("gf2_weight_rows_narrow_kernel", 9 * 4 * 6 * 3)}
NOT_EMULATED = {
    "gf2_weight_rows_wide_kernel": "cross-lane",
    "gf2_weight_total_kernel": "cross-lane, LDS, barriers, atomics",
    "gf2_weight_cols_kernel": "LDS, barriers, atomics",
    "gf2_weight_fold_kernel": "LDS, barriers",
    "gf2_weight_select_count_kernel": "LDS, barriers",
    "gf2_weight_select_scan_kernel": "LDS, barriers",
    "gf2_weight_select_scatter_kernel": "LDS, barriers",
}
# the device helpers each of them calls: their text counts as the kernel's
HELPERS = {
    "gf2_weight_rows_wide_kernel": ["weight_row_partial", "weight_fold_lanes"],
    "gf2_weight_total_kernel": ["weight_row_partial"],
    "gf2_weight_cols_kernel": ["weight_band", "weight_load_block", "weight_csa8", "weight_flush"],
    "gf2_weight_fold_kernel": [],
    "gf2_weight_select_count_kernel": ["weight_matches", "weight_block_scan"],
    "gf2_weight_select_scan_kernel": ["weight_block_scan"],
    "gf2_weight_select_scatter_kernel": ["weight_matches", "weight_block_scan"],
}
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
    return kernel_text.extract_all(words, SHARED) + "\n" + kernel_text.extract_all(os.path.join(WEIGHT, "gf2_weight.hip"), PIECES)


def sources():
    return sorted(glob.glob(os.path.join(WEIGHT, "*.hip")) + glob.glob(os.path.join(WEIGHT, "*.inc")))


def test_every_weight_kernel_is_classified():
    srcs = sources()
    assert [os.path.basename(s) for s in srcs] == ["gf2_weight.hip"]
    names = [k for path in srcs for k in kernel_text.global_kernels(path)]
    assert len(names) == len(set(names)) == 8, names
    assert not set(EMULATED) & set(NOT_EMULATED)
    missing = set(names) - set(EMULATED) - set(NOT_EMULATED)
    assert not missing, "new kernels: give each a driver in tests/weight_emu.cpp or a reason in NOT_EMULATED: %s" % sorted(missing)
    gone = (set(EMULATED) | set(NOT_EMULATED)) - set(names)
    assert not gone, "listed here, but no longer in csrc/weight: %s" % sorted(gone)
    for name, reason in NOT_EMULATED.items():
        for word in reason.split(", "):
            assert word in RULE_WORDS, (name, word)
    assert set(EMULATED) <= set(PIECES), "emulated, but not cut out of its file"
    assert "gf2_weight_rows_narrow_kernel" in EMULATED   # the LPN shape's kernel stays a word-level kernel
    assert set(HELPERS) == set(NOT_EMULATED)
    # no name twice across the library: the lists of tests/test_kernels_cpu.py, tests/test_gather_kernels_cpu.py and this one describe
    # one set of kernels
    csrc = os.path.dirname(WEIGHT)
    older = [k for pat in ("*.hip", "*.inc", "gather/*.hip", "gather/*.inc") for p in sorted(glob.glob(os.path.join(csrc, pat)))
             for k in kernel_text.global_kernels(p)]
    assert len(older) > 50 and not set(older) & set(names)


def test_the_reasons_match_the_text():
    """an emulated kernel shows none of the signs; a kernel that is not emulated shows each sign its reason names"""
    path = sources()[0]
    whole = kernel_text.mask(open(path).read())
    assert not re.search(SIGNS["inline assembly"], whole)   # builtins and plain C++ only
    for name in EMULATED:
        text = kernel_text.mask(pieces_text())
        for word, sign in SIGNS.items():
            assert not re.search(sign, text), (name, word)
    for name, reason in NOT_EMULATED.items():
        text = kernel_text.mask(kernel_text.extract_all(path, [name] + HELPERS[name]))
        for word in reason.split(", "):
            assert re.search(SIGNS[word], text), (name, word)


def test_narrow_row_kernel_touches_only_words_of_its_operand(tmp_path):
    body = tmp_path / "weight_body.inc"
    body.write_text(pieces_text())
    exe = tmp_path / "weight_emu"
    build = subprocess.run(["g++"] + FLAGS + ['-DKERNEL_BODY="%s"' % body, "-I", HERE, "-o", str(exe), os.path.join(HERE, "weight_emu.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-6000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    assert "all ok" in run.stdout, run.stdout
    counts = {label: int(n) for label, n in re.findall(r"^(.+): (\d+) cases ok$", run.stdout, re.M)}
    for kernel, (label, n) in EMULATED.items():
        assert counts.get(label) == n, (kernel, counts)


def test_hazard_audit_of_the_weight_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import asm_hazards
    finally:
        sys.path.pop(0)
    findings, stats = asm_hazards.audit(sources=[s for s in sources() if s.endswith(".hip")])
    assert stats["functions"] >= 8 and stats["instructions"] > 1000, stats
    assert stats["asm_instructions"] == 0, stats   # builtins and plain C++ only
    assert not findings, findings
