"""Device-resident triangular solves (gf2_trsm_dev) next to the product of the same size (gf2_mul_dev n x n x n).

    python tools/trsm_bench.py [--sizes 4096,16384,65536] [--reps 3] [--block D]

T is random unit triangular (a random matrix: only its strict triangle is read), B is n x n.  One JSON line per size: median wall
times in ms of the four variants and of the product, and each variant's ratio to the product (a triangular solve has half the bit
operations of that product).  --block sets M4RI_HIP_TRSM_BLOCK (64, 128, 256 or 512) for the run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--block", type=int, default=0, help="0: the library's block size")
    args = ap.parse_args()
    if args.block:
        os.environ["M4RI_HIP_TRSM_BLOCK"] = str(args.block)
    import __graft_entry__ as ge
    ge.build()
    from m4ri_rust_amd import device
    device.require_gpu()
    for n in [int(s) for s in args.sizes.split(",")]:
        T, src = device.DMat.random(n, n, 1), device.DMat.random(n, n, 2)
        B, C = device.DMat(n, n), device.DMat(n, n)

        def timed(fn):
            ts = []
            for _ in range(args.reps + 1):
                device.add(src, device.add(src, src), C=B)  # B = a copy of src
                device.equal(B, B)  # drain the queue
                t0 = time.perf_counter()
                fn()
                device.equal(C, C)  # the calls are asynchronous: wait for the stream
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts[1:])

        out = {"n": n, "block": args.block or "default"}
        out["mul_ms"] = round(timed(lambda: device.mul(T, src, C=C)), 3)
        for upper in (False, True):
            for right in (False, True):
                key = ("upper" if upper else "lower") + "_" + ("right" if right else "left")
                out[key + "_ms"] = round(timed(lambda: device.trsm(T, B, upper=upper, right=right)), 3)
                out[key + "_over_mul"] = round(out[key + "_ms"] / out["mul_ms"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
