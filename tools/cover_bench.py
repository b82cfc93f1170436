"""The covering-code reduction on the device (gf2_cover_reduce_dev) next to a plain copy of the pool's bytes and next to the host route
it replaces.

    python tools/cover_bench.py [--reps 20] [--warmup 3] [--small] [--out profiles/cover_bench.txt]

Pools of 256 columns, N = 2^20 and 2^26 rows of random bits, two segment lists:
  golay    ten Golay23 blocks and one Identity(1) from column 20 on: 231 bits -> 121 (two words of D);
  hamming  36 Hamming(3) blocks from column 2 on: 252 bits -> 144 (three words of D).
For every (N, list), in one run:
  cover          gf2_cover_reduce_dev with dist, the kernel the plan chooses;
  cover_no_dist  the same without dist;
  staged, global the launcher (csrc/cover/gf2_cover.h) with either kernel: the window words of a workgroup's rows copied into LDS by a
                 lane per word, or every lane reading the words of its row from global memory (one lane per 32-byte row);
  pool_copy      gf2_copy_block_dev of the pool's bytes.  The floor of the reduction is one read of P plus one write of D: 48 of the
                 copy's 64 bytes per row for golay, 56 for hamming (dist adds 4).
At N = 2^20 also the host route, once per list: download, the numpy reduction of tests/cover_ref.py, upload.

One process; every launch is timed on its own with HIP events after --warmup launches, the figure is the median of --reps launches, and
the variants of an (N, list) alternate launch by launch so that they see the same machine.  The pools rotate through as many buffers
as it takes to hold 768 MiB (at least three), so that no launch finds its data in the 256 MiB last-level cache.  One JSON line per
(N, list); --out keeps the run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not rates)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cover_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cover_ref as cr
    from m4ri_rust_amd import device
    device.require_gpu()
    L = device._lib.lib()
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    k_cover = L.gf2k_cover_reduce
    k_cover.restype, k_cover.argtypes = I, [P, LL, I, I, I, P, I, P, I, P, P, LL, P, I, P]
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    def ok(rc):
        assert rc == 0, "the launcher returned hipError %d" % rc

    def timed_together(launches):
        """{name: (median, min, max) in ms} of launches[name](i): the variants alternate, one event pair around every launch"""
        ts = {k: [] for k in launches}
        for i in range(args.warmup + args.reps):
            for name, launch in launches.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(i)
                b.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[name].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    C = device.CoverCode
    lists = {"golay": (20, [C.golay23()] * 10 + [C.identity(1)], [cr.golay23()] * 10 + [cr.identity(1)]),
             "hamming": (2, [C.hamming(3)] * 36, [cr.hamming(3)] * 36)}
    Ns = [1 << 12] if args.small else [1 << 20, 1 << 26]
    ld = NCOLS // 64
    for N in Ns:
        rot = 3 if args.small else max(3, -(-(768 << 20) // (N * 32)))
        tensors = [torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(rot)]
        pools = [device.DMat.from_torch(t, NCOLS) for t in tensors]
        for i, p in enumerate(pools):
            p.fill_random(40 + i)
        copy_dst = device.DMat(N, NCOLS)
        dist = torch.zeros(N, dtype=torch.int32, device="cuda")
        pool = lambda i: pools[i % rot]  # noqa: E731
        for name, (c0, segments, ref_segments) in lists.items():
            K, bits = sum(c.k for c in segments), sum(c.n for c in segments)
            dst = device.DMat(N, K)
            plan = device.cover_plan(N, NCOLS, segments)
            codes, arr, seg = device._cover_args(segments)
            tables = (ctypes.c_void_p * len(codes))(*[c.table_ptr() for c in codes])

            def kernel(variant):
                return lambda i: ok(k_cover(pool(i).s.data, ld, N, NCOLS, c0, arr, len(codes), seg, len(segments), tables, dst.s.data, dst.ld,
                                            dist.data_ptr(), variant, None))

            launches = {
                "cover": lambda i: device.cover_reduce(pool(i), c0, segments, D=dst, dist=dist.data_ptr()),
                "cover_no_dist": lambda i: device.cover_reduce(pool(i), c0, segments, D=dst, dist=device.SKIP),
                "staged": kernel(1),
                "global": kernel(0),
                "pool_copy": lambda i: device.copy_block(copy_dst, 0, 0, pool(i), 0, 0, N, NCOLS),
            }
            t = timed_together(launches)
            torch.cuda.synchronize()
            moved = N * (8 * ((c0 + bits + 63) // 64 - c0 // 64) + 8 * dst.ld + 4)
            res = {"what": "cover", "list": name, "N": N, "c0": c0, "segments": len(segments), "window_bits": bits, "K": K, "pool_bytes": N * 32,
                   "buffers": rot, "plan_variant": plan[0], "lanes_per_row_of_the_copy": plan[4], "lds_bytes": plan[2], "workgroups": plan[8]}
            for key, (med, lo, hi) in t.items():
                res[key + "_ms"] = round(med, 4)
                res[key + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            res["cover_over_pool_copy"] = round(t["cover"][0] / t["pool_copy"][0], 3)
            res["global_over_staged"] = round(t["global"][0] / t["staged"][0], 3)
            res["cover_GB_per_s"] = round(moved / t["cover"][0] / 1e6, 1)
            res["pool_copy_GB_per_s"] = round(N * 64 / t["pool_copy"][0] / 1e6, 1)
            res["cover_Grows_per_s"] = round(N / t["cover"][0] / 1e6, 2)
            emit(res)
            if N == Ns[0]:
                # the route the entry replaces, once: download, numpy, upload
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                words = pools[0].to_words()
                t1 = time.perf_counter()
                D_ref, dist_ref = cr.reduce(words, c0, ref_segments)
                t2 = time.perf_counter()
                up = device.DMat.from_words(D_ref, K)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                got, got_dist = device.cover_reduce(pools[0], c0, segments)
                same = bool(np.array_equal(got.to_words(), D_ref) and np.array_equal(got_dist.read(None), dist_ref))
                emit({"what": "host route", "list": name, "N": N, "download_ms": round(1e3 * (t1 - t0), 2), "numpy_ms": round(1e3 * (t2 - t1), 2),
                      "upload_ms": round(1e3 * (t3 - t2), 2), "total_ms": round(1e3 * (t3 - t0), 2), "same_bits_as_the_device": same})
                del up, got, got_dist, words, D_ref
            del dst
        del tensors, pools, copy_dst, dist
        torch.cuda.empty_cache()
        L.gf2_trim()
    with open(args.out, "w") as f:
        f.write("# python tools/cover_bench.py%s: reps %d, warmup %d\n" % (" --small" if args.small else "", args.reps, args.warmup))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
