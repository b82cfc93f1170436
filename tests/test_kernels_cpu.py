"""Every kernel of m4ri-rust_amd/csrc that needs no wave, no LDS, no barrier, no atomic and no inline assembly, run thread by thread on
the CPU under the host compiler's address and undefined-behaviour sanitizers (tests/kernels_emu.cpp behind tests/kernel_emu.h).  The text
that runs is the shipped text: tests/kernel_text.py cuts the named definitions out of the .hip files.  Buffers end with the last word of
the operand's last row, so a load or store of a word that holds no bit of the operand is a report, and the launchers' choice of 16-byte
accesses is judged by the alignment check over every parity of every row stride and base.  A GPU test can show neither.  No device is
needed.

The partition test keeps the two lists honest: a new __global__ kernel must be put into EMULATED (with a driver) or into NOT_EMULATED
(with the reason) before this file is green again."""
import glob
import os
import re
import subprocess

import kernel_text

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the part of gf2_kernels.hip that only development builds include (relative to CSRC, like the #include that names it)
DEV_THIN = os.path.join("..", "..", "tools", "gf2_kernels_dev_thin.inc")

# One program per group (built and run side by side: the three-level Strassen passes alone take the compiler half a minute).
# group -> file -> what is cut out of it, in the order the program needs it: constants, structs, helpers, kernels, launchers
PIECES = {
    "STREAM": [
        ("gf2_kernels.h", ["gf2k_mul_args"]),
        ("gf2_kernels.hip", [
            "xor4", "grid_for", "kTileWords7", "v8_tile", "v8_decode",
            "gf2_streamk_reduce_kernel", "gf2_packA_kernel", "gf2_splitk_reduce_kernel", "gf2_rowparity_kernel", "gf2_xor2d_kernel",
            "gf2_padcopy_kernel", "gf2_fill_random_kernel",
            "gf2k_packA", "gf2k_rowparity", "gf2k_xor2d", "gf2k_padcopy", "gf2k_fill_random",
        ]),
        (DEV_THIN, ["gf2_packB_kernel", "gf2k_packB_chunks", "gf2k_packB"]),  # development builds only
    ],
    "STRASSEN": [
        ("gf2_kernels.hip", [
            "xor4", "static_for_impl", "static_for", "grid_for",
            "gf2_strassen_split_kernel", "nt_load4", "nt_store4", "gf2_strassen_merge_kernel",
            "strassen_combo", "gf2_strassen_split2_kernel", "strassen_fold", "gf2_strassen_merge2_kernel",
            "gf2k_split3_srcs", "kStrassenSupp", "gf2_strassen_split3_kernel", "kStrassenFoldTo", "gf2_strassen_merge3_kernel",
            "gf2k_strassen_split", "gf2k_strassen_split2", "gf2k_strassen_split3",
            "gf2k_strassen_merge", "gf2k_strassen_merge2", "gf2k_strassen_merge3",
        ]),
    ],
    "REST": [
        ("gf2_kernels.h", ["gf2k_elim_state"]),
        ("gf2_ple.hip", ["ple_panel_apply", "ple_gather", "ple_compose", "ple_compress_extract", "ple_compress_place", "ple_tri"]),
        ("gf2_trsm.hip", ["trsm_copy_back"]),
        ("gf2_nullspace.hip", ["CTL_WORDS", "low_bits", "compress", "nullspace_prepare", "nullspace_assemble"]),
        ("gf2_elim.hip", [
            "gf2_elim_gather_kernel", "gf2_elim_scatter_kernel", "gf2_elim_begin_block_kernel", "gf2_elim_toggle_kernel",
            "gf2_set_diag_kernel", "gf2_scatter_rows_kernel", "gf2k_elim_begin_block", "gf2k_set_diag", "gf2k_scatter_rows",
        ]),
    ],
}

# the kernels that run on the CPU: one line of the program's output each, with its case count
EMULATED = {
    "gf2_copy_block_kernel": None,  # tests/test_blocks_kernel_cpu.py
    "gf2_xor2d_kernel": ("gf2_xor2d_kernel", 7590),
    "gf2_padcopy_kernel": ("gf2_padcopy_kernel", 10152),
    "gf2_fill_random_kernel": ("gf2_fill_random_kernel", 846),
    "gf2_packA_kernel": ("gf2_packA_kernel", 576),
    "gf2_splitk_reduce_kernel": ("gf2_splitk_reduce_kernel", 1104),
    "gf2_streamk_reduce_kernel": ("gf2_streamk_reduce_kernel", 360),
    "gf2_rowparity_kernel": ("gf2_rowparity_kernel", 6768),
    "gf2_packB_kernel": ("gf2_packB_kernel", 480),
    "gf2_strassen_split_kernel": ("gf2_strassen_split_kernel", 28),
    "gf2_strassen_split2_kernel": ("gf2_strassen_split2_kernel", 28),
    "gf2_strassen_split3_kernel": ("gf2_strassen_split3_kernel", 35),
    "gf2_strassen_merge_kernel": ("gf2_strassen_merge_kernel", 32),
    "gf2_strassen_merge2_kernel": ("gf2_strassen_merge2_kernel", 32),
    "gf2_strassen_merge3_kernel": ("gf2_strassen_merge3_kernel", 40),
    "ple_panel_apply": ("ple_panel_apply", 504),
    "ple_gather": ("ple_gather", 5076),
    "ple_compose": ("ple_compose", 18),
    "ple_compress_extract": ("ple_compress_extract + ple_compress_place", 3900),
    "ple_compress_place": ("ple_compress_extract + ple_compress_place", 3900),
    "ple_tri": ("ple_tri", 2592),
    "trsm_copy_back": ("trsm_copy_back", 1692),
    "nullspace_prepare": ("nullspace_prepare + nullspace_assemble", 780),
    "nullspace_assemble": ("nullspace_prepare + nullspace_assemble", 780),
    "gf2_elim_gather_kernel": ("gf2_elim_gather_kernel + gf2_elim_scatter_kernel", 159),
    "gf2_elim_scatter_kernel": ("gf2_elim_gather_kernel + gf2_elim_scatter_kernel", 159),
    "gf2_elim_toggle_kernel": ("gf2_elim_toggle_kernel + gf2_set_diag_kernel + gf2_scatter_rows_kernel + gf2_elim_begin_block_kernel", 334),
    "gf2_set_diag_kernel": ("gf2_elim_toggle_kernel + gf2_set_diag_kernel + gf2_scatter_rows_kernel + gf2_elim_begin_block_kernel", 334),
    "gf2_scatter_rows_kernel": ("gf2_elim_toggle_kernel + gf2_set_diag_kernel + gf2_scatter_rows_kernel + gf2_elim_begin_block_kernel", 334),
    "gf2_elim_begin_block_kernel": ("gf2_elim_toggle_kernel + gf2_set_diag_kernel + gf2_scatter_rows_kernel + gf2_elim_begin_block_kernel", 334),
}

# the others, each with the words of the scope rule that keep it off the CPU
NOT_EMULATED = {
    "ple_panel_scan": "cross-lane",
    "ple_panel_pivots": "cross-lane",
    "trsm_invert_blocks": "LDS, barriers",
    "gf2_m4rm_kernel_v3": "LDS, barriers, cross-lane, inline assembly",
    "gf2_m4rm_kernel_v6": "LDS, barriers, cross-lane, inline assembly",
    "gf2_m4rm_kernel_v8": "LDS, barriers, cross-lane, inline assembly",
    "gf2_narrow_kernel": "LDS, barriers",
    "gf2_widevec_kernel": "cross-lane, LDS, barriers",
    "gf2_tallskinny3_kernel": "LDS, barriers",
    "gf2_tallskinny5_kernel": "LDS, barriers",
    "gf2_tallskinny6_kernel": "LDS, barriers",
    "gf2_tallskinny7_kernel": "LDS, barriers",
    "gf2_tallskinny4_kernel": "LDS, barriers, atomics",
    "gf2_va_kernel": "LDS, barriers, atomics",
    "gf2_diff_kernel": "cross-lane, atomics",
    "gf2_transpose_kernel": "cross-lane",
    "gf2_transpose512_kernel": "LDS, barriers, cross-lane",
    "gf2_lpn8_kernel": "LDS, barriers, cross-lane",
    "gf2_lpnvec_kernel": "LDS, barriers, cross-lane",
    "gf2_lpn256_kernel": "LDS, barriers, cross-lane",
    "gf2_elim_pivot_kernel": "LDS, barriers, cross-lane",
    "gf2_elim_update_kernel": "LDS, barriers, atomics",
    "gf2_elim_plan_kernel": "LDS, barriers",
    "gf2_elim_lastword_kernel": "cross-lane, atomics",
    "gf2_any_nonzero_kernel": "cross-lane, atomics",
    "gf2_elim_small_kernel": "LDS, barriers",
    "gf2_elim_batch_wave_kernel": "cross-lane",
    "gf2_elim_batch_lds_kernel": "LDS, barriers",
}

RULE_WORDS = {"cross-lane", "LDS", "barriers", "atomics", "inline assembly"}


def kernel_sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc"))) + [os.path.join(CSRC, DEV_THIN)]


def test_every_kernel_is_classified():
    names = [k for path in kernel_sources() for k in kernel_text.global_kernels(path)]
    assert len(names) == len(set(names)), "a kernel name twice: %s" % sorted(n for n in names if names.count(n) > 1)
    assert len(names) >= 58, names  # 55 in the .hip files and 3 in gf2_lpn.inc when this test was written
    both = set(EMULATED) & set(NOT_EMULATED)
    assert not both, "classified twice: %s" % sorted(both)
    missing = set(names) - set(EMULATED) - set(NOT_EMULATED)
    assert not missing, "new kernels: give each a driver in tests/kernels_emu.cpp or a reason in NOT_EMULATED: %s" % sorted(missing)
    gone = (set(EMULATED) | set(NOT_EMULATED)) - set(names)
    assert not gone, "listed here, but no longer in csrc: %s" % sorted(gone)
    for name, reason in NOT_EMULATED.items():
        for word in reason.split(", "):
            assert word in RULE_WORDS, (name, word)
    cut = {n for group in PIECES.values() for _, ns in group for n in ns}
    assert not (set(EMULATED) - {"gf2_copy_block_kernel"}) - cut, "emulated, but not cut out of its file"


def make_list(path, var):
    """the words of `var := ...` in a makefile, continuation lines joined"""
    with open(path) as f:
        text = f.read().replace("\\\n", " ")
    return re.search(r"^%s\s*:?=(.*)$" % var, text, re.M).group(1).split()


def test_every_included_inc_is_a_dependency_of_the_build():
    """gf2_kernels.hip includes text from other files (today gf2_lpn.inc and, in development builds, four files under tools/): an edit
    of such a file rebuilds the library only if it is in LIB_HDR (csrc/sources.mk) or, for one under tools/, in DEV_DEPS
    (tools/Makefile).  Whatever is cut out of gf2_kernels.hip later is held to the same rule by the walk below."""
    root = os.path.dirname(HERE)
    tools = os.path.join(root, "tools")
    parts, todo = [], [os.path.join(CSRC, "gf2_kernels.hip")]
    while todo:
        path = todo.pop()
        with open(path) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+\.inc)"', f.read(), re.M):
                p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
                assert os.path.isfile(p), (path, inc)
                if p not in parts:
                    parts.append(p)
                    todo.append(p)
    lib_hdr = {os.path.normpath(os.path.join(CSRC, w)) for w in make_list(os.path.join(CSRC, "sources.mk"), "LIB_HDR")}
    dev_deps = {os.path.normpath(os.path.join(tools, w)) for w in make_list(os.path.join(tools, "Makefile"), "DEV_DEPS") if "$" not in w}
    assert len(parts) >= 5, parts  # gf2_lpn.inc and four files of development builds when this test was written
    for p in parts:
        assert p in (dev_deps if os.path.dirname(p) == tools else lib_hdr), "%s: not a dependency of the build" % os.path.relpath(p, root)


def build_body(tmp_path, group):
    body = tmp_path / ("kernels_body_%s.inc" % group)
    parts = []
    for fname, names in PIECES[group]:
        parts.append("// ---- %s\n" % fname)
        parts.append(kernel_text.extract_all(os.path.join(CSRC, fname), names))
    body.write_text("".join(parts))
    return body


def test_kernels_touch_only_words_of_their_operands(tmp_path):
    with open(os.path.join(CSRC, "gf2_kernels.h")) as f:
        pivots = re.search(r"\bGF2K_ELIM_BLOCK_PIVOTS\s*=\s*(\d+)", f.read()).group(1)
    builds = []
    for group in PIECES:
        exe = tmp_path / ("kernels_emu_" + group)
        cmd = ["g++"] + FLAGS + ["-DEMU_" + group, '-DKERNEL_BODY="%s"' % build_body(tmp_path, group), "-DGF2K_ELIM_BLOCK_PIVOTS=" + pivots,
                                 "-I", CSRC, "-I", HERE, "-o", str(exe), os.path.join(HERE, "kernels_emu.cpp")]
        builds.append((exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    runs = []
    for exe, proc in builds:
        out = proc.communicate()[0]
        assert proc.returncode == 0, out[-6000:]
        runs.append(subprocess.Popen([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    stdout = ""
    for proc in runs:
        out, err = proc.communicate()
        assert proc.returncode == 0, out[-2000:] + err[-6000:]
        assert "all ok" in out, out
        stdout += out
    counts = {label: int(n) for label, n in re.findall(r"^(.+): (\d+) cases ok$", stdout, re.M)}
    for kernel, line in EMULATED.items():
        if line is not None:
            assert counts.get(line[0]) == line[1], (kernel, line, counts)


# ---- the extractor's own tests

SAMPLE = r'''
#include <x>
namespace {
// helper { with a brace in a comment
__device__ __forceinline__ int helper(int a) {
  const char *s = "}{";  /* } */
  if (a) { a += '{'; }
  return a;
}
int helper2(int a);  // a declaration
template <int N, bool B = false>
__global__ __launch_bounds__(256) void kern(int *p, int n) {
  for (int i = 0; i < n; ++i) { if (i) { p[i] = helper(i); } }
}
struct args { int a[7]; };
constexpr int TABLE[2][2] = {{1, 2}, {3, 4}};
}  // namespace
extern "C" int launch(int *p) {
  hipLaunchKernelGGL((kern<1, true>), 1, 1, 0, 0, p, 3);
  return helper2(1);
}
int twice(int a) { return a; }
int twice(long a) { return (int)a; }
'''


def sample(tmp_path):
    p = tmp_path / "sample.hip"
    p.write_text(SAMPLE)
    return str(p)


def test_extract_nested_braces_strings_and_comments(tmp_path):
    text = kernel_text.extract(sample(tmp_path), "helper")
    assert text.startswith("__device__ __forceinline__ int helper(int a) {") and text.rstrip().endswith("return a;\n}")
    assert '"}{"' in text and "'{'" in text


def test_extract_template_kernel_launcher_struct_and_table(tmp_path):
    path = sample(tmp_path)
    text = kernel_text.extract(path, "kern")
    assert text.startswith("template <int N, bool B = false>\n__global__") and text.count("{") == text.count("}") == 3
    assert kernel_text.extract(path, "launch").startswith('extern "C" int launch(int *p) {')
    assert kernel_text.extract(path, "args") == "struct args { int a[7]; };\n"
    assert kernel_text.extract(path, "TABLE") == "constexpr int TABLE[2][2] = {{1, 2}, {3, 4}};\n"
    assert kernel_text.global_kernels(path) == ["kern"]


def test_extract_refuses_missing_and_double(tmp_path):
    import pytest
    path = sample(tmp_path)
    with pytest.raises(KeyError):
        kernel_text.extract(path, "helper2")  # declared and called, never defined
    with pytest.raises(KeyError):
        kernel_text.extract(path, "nothing")
    with pytest.raises(ValueError):
        kernel_text.extract(path, "twice")
