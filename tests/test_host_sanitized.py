"""The host units of the library -- mzd_host, gf2_small_host, ple_host, trsm_host, nullspace_host -- under the host compiler's address,
leak and undefined-behaviour sanitizers, as a stand-alone program (tests/cpp/host_san.cpp with the stubs of tests/cpp/host_san_stubs.cpp,
linked with the C oracle as the reference).  These routines run in the caller's process, on its heap through rows[] and on windows of
its matrices; the other host tests reach them through ctypes, where no sanitizer watches.  Every gf2_*_host_small entry and every
container function runs over 11 x 11 shapes around the word boundaries, on plain matrices and on windows of dirty parents; results are
compared bit for bit, the parents bit by bit outside the window.  The overlap predicates of csrc/dev_args.h, which every device-resident
entry relies on, are checked in the same program against enumerated sets of bits and bytes.  No device is needed and none is used."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "m4ri-rust_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CXX = ["g++", "-std=c++17"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I", ORACLE]
UNITS = [os.path.join(CSRC, f) for f in ("mzd_host.cpp", "gf2_small_host.cpp", "ple_host.cpp", "trsm_host.cpp", "nullspace_host.cpp")]
UNITS += [os.path.join(HERE, "cpp", "host_san.cpp"), os.path.join(HERE, "cpp", "host_san_stubs.cpp")]

# what the program prints, one line per routine
CASES = {
    "gf2_echelonize_host_small full": 968,
    "gf2_echelonize_host_small": 968,
    "gf2_ple_host_small": 968,
    "gf2_trsm_host_small": 968,
    "gf2_nullspace_host_small": 968,
    "gf2_mul_host_small": 968,
    "gf2_mul_nt_host_small": 968,
    "mzd_init_window": 242,
    "mzd_copy": 484,
    "mzd_transpose": 484,
    "mzd_add / mzd_sub": 726,
    "mzd_concat": 484,
    "mzd_stack": 484,
    "mzd_submatrix": 484,
    "mzd_row_swap / mzd_copy_row": 242,
    "mzd_col_swap": 968,
    "mzd_row_clear_offset": 1694,
    "mzd_is_zero / mzd_equal": 242,
    "mzd_set_ui": 484,
    "mzd_make_table": 242,
    "mzd_invert_naive": 264,
    "mzd_apply_p / mzp": 1936,
    "gf2_mzd_save / gf2_mzd_load": 242,
    "pinned pool fallback": 1,
    "dev_args.h overlap predicates": 567630,
}


def test_host_routines_under_sanitizers(tmp_path):
    jobs = []
    for src in UNITS + [os.path.join(ORACLE, "gf2_oracle.c")]:
        obj = tmp_path / (os.path.basename(src) + ".o")
        cmd = (["gcc", "-std=c11"] + SAN + ["-I", ORACLE] if src.endswith(".c") else CXX) + ["-c", src, "-o", str(obj)]
        jobs.append((obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for obj, proc in jobs:
        out = proc.communicate()[0]
        assert proc.returncode == 0, out[-6000:]
    exe = tmp_path / "host_san"
    subprocess.check_call(["g++"] + SAN + ["-o", str(exe)] + [str(obj) for obj, _ in jobs] + ["-lm"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("M4RI_HIP_")}  # the library's own defaults
    run = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    assert "all ok" in run.stdout, run.stdout
    counts = {name: int(n) for name, n in re.findall(r"^(.+): (\d+) cases ok$", run.stdout, re.M)}
    assert counts == CASES
