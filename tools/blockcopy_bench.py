"""Device block copy (gf2_copy_block_dev) next to a plain device-to-device copy of the same bytes, and gf2_solve_left_dev next to the
elimination of the same augmented matrix.

    python tools/blockcopy_bench.py [--n 65536] [--solve-n 32768] [--reps 20] [--no-solve]

Block copy: an n x n rectangle in three placements -- (a) fully aligned (sc = dc = 0), (b) sc % 64 = 0 into dc % 64 = 37, (c) sc % 64 = 37
into dc % 64 = 0 with both word offsets odd (sc = 101, dc = 64).  Every launch is timed on its own with HIP events after --warmup
launches; the figure is the median of --reps launches.  Sources and destinations rotate through three buffers each (n = 65536: 514 MiB a
buffer, more than the 256 MiB of the last-level cache), so no launch finds its input or its output in a cache.  The plain copy of the
same run moves the same 2 * n * n / 8 bytes, once as a contiguous torch copy_ and once as a copy_ between strided views with the
rectangle's geometry; the ratio is taken against the faster of the two.  After the timing every placement is checked: the block is
copied back to offset 0 of a fresh buffer and compared with the source rectangle by gf2_equal_dev.

Solve: A (n x n, random) X = B with 64 and with n right-hand-side columns, device resident, against gf2_echelonize_dev (reduced form,
limit n) of the same [A | B], operands cloned outside the timed region; the difference is what the assembly on the device costs (two
block copies in, the clear and the scatter of B, one block copy back).  Median of --solve-reps after one warm-up.
One JSON line per measurement; profiles/blockcopy_bench.txt keeps a run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROT = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--solve-n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--no-copy", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from m4ri_rust_amd import device
    device.require_gpu()

    def timed(launch, reps, warmup):
        """median event time in ms of launch(i), i counting up through warm-up and repetitions"""
        ts = []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(i)
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ts.append(a.elapsed_time(b))
        return statistics.median(ts), min(ts), max(ts)

    if not args.no_copy:
        n = args.n
        w = n // 64
        ld = w + 4  # room for the offsets; even
        cols = ld * 64
        src_t = [torch.empty((n, ld), dtype=torch.int64, device="cuda") for _ in range(ROT)]
        dst_t = [torch.zeros((n, ld), dtype=torch.int64, device="cuda") for _ in range(ROT)]
        src = [device.DMat.from_torch(t, cols) for t in src_t]
        dst = [device.DMat.from_torch(t, cols) for t in dst_t]
        for i, s in enumerate(src):
            s.fill_random(100 + i)
        nbytes = 2 * n * w * 8
        plain = {}
        flat_a = [torch.empty(n * w, dtype=torch.int64, device="cuda") for _ in range(ROT)]
        flat_b = [torch.ones(n * w, dtype=torch.int64, device="cuda") for _ in range(ROT)]
        plain["contiguous"] = timed(lambda i: flat_a[i % ROT].copy_(flat_b[i % ROT]), args.reps, args.warmup)
        del flat_a, flat_b
        plain["strided"] = timed(lambda i: dst_t[i % ROT][:, :w].copy_(src_t[i % ROT][:, :w]), args.reps, args.warmup)
        best = min(plain, key=lambda k: plain[k][0])
        for k, (med, lo, hi) in plain.items():
            print(json.dumps({"what": "plain copy_, " + k, "n": n, "bytes": nbytes, "ms": round(med, 4), "ms_min": round(lo, 4),
                              "ms_max": round(hi, 4), "TBps": round(nbytes / med / 1e9, 3)}), flush=True)
        for name, sc, dc in (("a: aligned", 0, 0), ("b: sc%64=0 -> dc%64=37", 0, 37), ("c: sc%64=37 -> dc%64=0, odd words", 101, 64)):
            med, lo, hi = timed(lambda i: device.copy_block(dst[i % ROT], 0, dc, src[i % ROT], 0, sc, n, n), args.reps, args.warmup)
            back = device.DMat(n, n)
            device.copy_block(back, 0, 0, dst[0], 0, dc, n, n)
            want = device.submatrix(src[0], 0, sc, n, sc + n)
            same = device.equal(back, want)
            del back, want
            print(json.dumps({"what": "gf2_copy_block_dev, " + name, "n": n, "sc": sc, "dc": dc, "bytes": nbytes, "ms": round(med, 4),
                              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "TBps": round(nbytes / med / 1e9, 3),
                              "rate_over_plain_copy": round(plain[best][0] / med, 3), "plain_copy": best, "same_bits": bool(same)}),
                  flush=True)
        del src, dst, src_t, dst_t
        torch.cuda.empty_cache()

    if not args.no_solve:
        n = args.solve_n
        A0 = device.DMat.random(n, n, 7)
        for k in (64, n):
            B0 = device.DMat.random(n, k, 8)
            T0 = device.concat(A0, B0)
            held = {}

            def solve(i):
                device.solve_left(held["A"], held["B"], check=True)

            def elim(i):
                device.echelonize(held["T"], full=True, ncols_limit=n)

            def run(fn, prepare):
                ts = []
                for i in range(1 + args.solve_reps):
                    held.clear()
                    prepare()
                    ts.append(timed(fn, 1, 0)[0])
                return statistics.median(ts[1:])
            t_solve = run(solve, lambda: held.update(A=A0.clone(), B=B0.clone()))
            t_elim = run(elim, lambda: held.update(T=T0.clone()))
            held.clear()
            print(json.dumps({"what": "gf2_solve_left_dev", "m": n, "n": n, "rhs_columns": k, "solve_ms": round(t_solve, 3),
                              "echelonize_ms": round(t_elim, 3), "assembly_ms": round(t_solve - t_elim, 3),
                              "assembly_share": round((t_solve - t_elim) / t_solve, 4)}), flush=True)
            del B0, T0


if __name__ == "__main__":
    main()
