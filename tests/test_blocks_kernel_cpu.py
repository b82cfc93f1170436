"""The block-copy kernel (m4ri-rust_amd/csrc/gf2_blocks.hip) run thread by thread on the CPU under the host compiler's address and
undefined-behaviour sanitizers (tests/blocks_emu.cpp): 8424 rectangles over source offset x destination offset x width x plain /
accumulate / cleared tail x even and odd word positions x even and odd row strides x 16- and 8-byte aligned bases, in buffers that end
with the rectangle, and 2^20 + 1 rows of 65 columns for the launch shape.  A load or store of a word that holds no bit of the rectangle
is a sanitizer report; a GPU test could show it only by faulting.  No device is needed."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "m4ri-rust_amd", "csrc", "gf2_blocks.hip")


def test_kernel_touches_only_words_of_the_rectangle(tmp_path):
    body = tmp_path / "kernel_body.inc"
    body.write_text("".join(ln for ln in open(KERNEL) if not ln.startswith("#include")))
    exe = tmp_path / "blocks_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           '-DKERNEL_BODY="%s"' % body, "-o", str(exe), os.path.join(HERE, "blocks_emu.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "8424 cases ok" in run.stdout and "tall ok, grid 8193 x 1 block 2 x 128" in run.stdout, run.stdout
