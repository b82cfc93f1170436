"""Device-resident PLE / PLUQ (gf2_ple_dev) next to gf2_echelonize_dev(full=0) on the same matrices.

    python tools/ple_bench.py [--sizes 4096,16384,65536] [--reps 3] [--rank R]

One JSON line per size: median wall times in ms (the device calls are synchronous), ranks and the ratio PLE / echelon."""
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
    ap.add_argument("--rank", type=int, default=0, help="0: random (full rank); else the rank of a product X Y")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from m4ri_rust_amd import device
    device.require_gpu()
    for n in [int(s) for s in args.sizes.split(",")]:
        if args.rank:
            src = device.mul(device.DMat.random(n, args.rank, 1), device.DMat.random(args.rank, n, 2))
        else:
            src = device.DMat.random(n, n, 1)

        def fresh():
            return device.add(src, device.add(src, src))  # a copy of src

        def timed(fn):
            ts = []
            for _ in range(args.reps + 1):
                A = fresh()
                device.equal(A, A)  # drain the queue
                t0 = time.perf_counter()
                res = fn(A)
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts[1:]), res

        t_ple, (r_ple, _, q_ple) = timed(lambda A: device.ple(A, pluq=False))
        t_pluq, (r_pluq, _, q_pluq) = timed(lambda A: device.ple(A, pluq=True))
        t_ech, (r_ech, piv) = timed(lambda A: device.echelonize(A, full=False))
        # a cheap consistency check (tests/test_gpu_ple.py checks the factors): rank and Q against the echelon form
        assert r_ple == r_pluq == r_ech and q_ple[:r_ech] == q_pluq[:r_ech] == piv, "PLE disagrees with gf2_echelonize_dev"
        print(json.dumps({"n": n, "rank_arg": args.rank, "ple_ms": round(t_ple, 2), "pluq_ms": round(t_pluq, 2),
                          "echelonize_full0_ms": round(t_ech, 2), "rank": r_ple, "rank_pluq": r_pluq, "rank_ech": r_ech,
                          "ple_over_ech": round(t_ple / t_ech, 2)}), flush=True)


if __name__ == "__main__":
    main()
