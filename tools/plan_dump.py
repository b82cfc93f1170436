#!/usr/bin/env python3
"""Prints every query of the launch planner over a fixed grid of shapes, and a SHA-256 of the whole dump:
     python tools/plan_dump.py [path/to/libm4ri_hip.so] [--quiet]
The planner is pure host arithmetic, so two builds that plan alike give the same digest on any machine; without a visible device
gf2_strassen_levels is the model's answer too.  After a change that must not move a plan (a refactor of mul_plan_host.cpp) compare
the digests of the two builds; when they differ, diff the dumps: the line names the query and the shape.  Doubles are float.hex()."""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1, 8, 9, 64, 128, 129, 256, 257, 512, 1000, 1024, 2048, 2049, 4096, 4160, 8192, 12700, 16384, 17000, 32768, 40000, 65536, 70000)
L = (1, 64, 70, 256, 257, 1000, 2048, 4096, 7000, 8192, 16384, 33000, 65536)
N = (1, 8, 64, 65, 128, 257, 512, 600, 1000, 2048, 4096, 16384, 40000, 65536)


def main():
    args = [a for a in sys.argv[1:] if a != "--quiet"]
    lib = ctypes.CDLL(args[0] if args else os.path.join(ROOT, "m4ri-rust_amd", "lib", "libm4ri_hip.so"))
    I = ctypes.c_int
    lib.gf2_tile_plan.restype = lib.gf2_model_time.restype = lib.gf2_strassen_pass_bytes.restype = ctypes.c_double
    lib.gf2_model_time.argtypes = lib.gf2_strassen_pass_bytes.argtypes = [I] * 4
    lib.gf2_mul_workspace_bytes.restype = ctypes.c_size_t
    t9, t5, d3, e12, kind = (ctypes.c_longlong * 9)(), (ctypes.c_longlong * 5)(), (I * 3)(), (ctypes.c_double * 12)(), I()
    digest, quiet = hashlib.sha256(), "--quiet" in sys.argv

    def out(*fields):
        line = " ".join(f.hex() if isinstance(f, float) else str(f) for f in fields) + "\n"
        digest.update(line.encode())
        if not quiet:
            sys.stdout.write(line)

    for m in M:
        for l in L:
            for n in N:
                for batch in (1, 7, 49, 343):
                    for packed in (0, 1):
                        t = lib.gf2_tile_plan(m, l, n, batch, packed, t9)
                        lib.gf2_tile_plan_band(m, l, n, batch, packed, t5)
                        out("tile", m, l, n, batch, packed, t, *t9, *t5)
                for algo in (0, 1, 2, 3):
                    for param in (0, 1, 3, 6):
                        lv = lib.gf2_mul_plan(m, l, n, algo, param, ctypes.byref(kind), d3)
                        out("mul", m, l, n, algo, param, lv, kind.value, *d3, lib.gf2_strassen_levels(m, l, n, algo, param),
                            lib.gf2_mul_workspace_bytes(m, l, n, algo, param))
                for lv in range(5):
                    out("model", m, l, n, lv, lib.gf2_model_time(m, l, n, lv), lib.gf2_strassen_pass_bytes(m, l, n, lv))
                for algo in (0, 1):
                    out("host", m, l, n, algo, lib.gf2_host_plan_model(m, l, n, algo, 0, e12), *e12)
    print("sha256", digest.hexdigest())


if __name__ == "__main__":
    main()
