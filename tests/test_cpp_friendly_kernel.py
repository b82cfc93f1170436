"""Builds and runs tests/cpp/test_friendly_kernel.cpp: BinMatrix::kernel() of include/m4ri_friendly.hpp over libm4ri_hip.so (g++
only: the header needs no HIP toolchain).  Compiling needs no device; the run does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "m4ri-rust_amd", "lib")


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_friendly_kernel")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_friendly_kernel.cpp"), "-o", out,
                           "-L", LIBDIR, "-lm4ri_hip", "-Wl,-rpath," + LIBDIR])
    return out


def test_cpp_kernel_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_kernel(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
