"""Builds and runs tests/cpp/test_streamk_cut.cpp: the stream-K cut that the launch planner (v8_model) and the tile-kernel launcher
(launch_v8) both take from m4ri-rust_amd/csrc/gf2_variants.h, over every (T, Q, n_rem, want) of a small range.  g++ only: the compile
is the proof that the shared header needs no HIP.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_streamk_cut_invariants(tmp_path):
    exe = str(tmp_path / "test_streamk_cut")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_streamk_cut.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
