"""One LF1 round of a BKW reduction on the device (gf2_lf1_reduce_dev) next to a plain copy of the pool's bytes and next to the route
that exists without the fused scatter kernel: the index arrays, then two gf2_gather_rows_dev passes.

    python tools/lf1_bench.py [--reps 20] [--warmup 3] [--small]

Pools of 256 columns, N = 2^20 and 2^26 rows of random bits, window c0 = 37, b = 8, 12, 13, 14, 15, 16, 20, 24; for every (N, b), in
one run:
  reduce      gf2_lf1_reduce_dev: memset, class firsts, count, scan, scatter;
  first, count, scan, scatter   its launches singly, through the library's launchers (csrc/bkw/gf2_bkw.h), on the state the launch
              before them left for the same pool (`first` on a table preset outside the timed span); where `first` is the LDS variant,
              first_global_atomics is the other class-first kernel on the same table;
  pool_copy   gf2_copy_block_dev of the pool's bytes: the reduction reads P once plus one random row per survivor and writes D once;
  two_gathers gf2_gather_rows_dev(D, P, src) then gf2_gather_rows_dev(D, P, partner, accumulate) on index arrays made beforehand;
              composed = first + count + scan + count + two_gathers is the least the route without the fused kernel costs: the second
              `count` stands for the launch that would write src and partner, which reads what the count kernel reads (the key and the
              table entry of every row) and writes 8 bytes per survivor on top;
  scatter_1_lane, scatter_2_lanes   the scatter kernel with one lane per row and with a lane per 16-byte piece (the plan's choice at
              four words);
At N = 2^20, b = 12 also the host route that the entry replaces, once: download, the numpy reference of tests/lf1_ref.py, upload.

One process; every launch is timed on its own with HIP events after --warmup launches, the figure is the median of --reps launches, and
the variants of an (N, b) alternate launch by launch so that they see the same machine.  The pools rotate through as many buffers as
it takes to hold 768 MiB (at least three), so that no launch finds its data in the 256 MiB last-level cache.  One JSON line per
(N, b); profiles/lf1_bench.txt keeps a run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS, C0 = 256, 37


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not rates)")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from m4ri_rust_amd import device
    device.require_gpu()
    L = device._lib.lib()
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    k_first, k_count, k_scan, k_scatter = L.gf2k_lf1_first, L.gf2k_lf1_count, L.gf2k_lf1_scan, L.gf2k_lf1_scatter
    for fn, argtypes in ((k_first, [P, LL, I, I, I, P, I, P]), (k_count, [P, LL, I, I, I, I, I, P, P, P]), (k_scan, [P, LL, P, P]),
                         (k_scatter, [P, LL, I, I, I, I, I, P, P, P, LL, I, P, I, P])):
        fn.restype, fn.argtypes = I, argtypes

    def ok(rc):
        assert rc == 0, "a launcher returned hipError %d" % rc

    def timed_together(launches, prepare):
        """{name: (median, min, max) in ms} of launches[name](i): the variants alternate, one event pair around every launch;
        prepare[name](i), where there is one, runs before the span"""
        ts = {k: [] for k in launches}
        for i in range(args.warmup + args.reps):
            for name, launch in launches.items():
                if name in prepare:
                    prepare[name](i)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(i)
                b.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[name].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    Ns = [1 << 12] if args.small else [1 << 20, 1 << 26]
    bs = [3, 14, 15] if args.small else [8, 12, 13, 14, 15, 16, 20, 24]
    ld = NCOLS // 64
    for N in Ns:
        rot = 3 if args.small else max(3, -(-(768 << 20) // (N * 32)))
        tensors = [torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(rot)]
        pools = [device.DMat.from_torch(t, NCOLS) for t in tensors]
        for i, p in enumerate(pools):
            p.fill_random(20 + i)
        dst = device.DMat(N, NCOLS)
        src = torch.zeros(N, dtype=torch.int32, device="cuda")
        count = torch.zeros(4, dtype=torch.int32, device="cuda")
        plan = device.lf1_plan(N, NCOLS, 8)
        rows, blocks = plan[3], plan[5] // 4
        counts = torch.zeros(blocks, dtype=torch.int32, device="cuda")
        for b in bs:
            first = torch.zeros(1 << b, dtype=torch.int32, device="cuda")
            # the index arrays of the composed route, made beforehand: the survivors and their partners, per pool
            idx = []
            for t, p in zip(tensors, pools):
                device.lf1_reduce(p, C0, b, D=dst, first=first.data_ptr(), count=count.data_ptr(), src=src.data_ptr())
                torch.cuda.synchronize()
                n = int(count[0])
                s = src[:n].clone()
                keys = (t[:, 0] >> C0) & ((1 << b) - 1)
                idx.append((n, s, first[keys[s.long()]].clone()))
                del keys
            variant = device.lf1_plan(N, NCOLS, b)[0]
            fp, cp, sp, kp = first.data_ptr(), count.data_ptr(), src.data_ptr(), counts.data_ptr()
            pool = lambda i: pools[i % rot]  # noqa: E731

            def two_gathers(i):
                n, s, partner = idx[i % rot]
                view = device.DMat.wrap(dst.s.data, n, NCOLS, dst.ld, keep=dst)
                device.gather_rows(pool(i), s.data_ptr(), D=view)
                device.gather_rows(pool(i), partner.data_ptr(), D=view, accumulate=True)

            launches = {
                "reduce": lambda i: device.lf1_reduce(pool(i), C0, b, D=dst, first=fp, count=cp, src=sp),
                "first": lambda i: ok(k_first(pool(i).s.data, ld, N, C0, b, fp, -1, None)),
                "count": lambda i: ok(k_count(pool(i).s.data, ld, N, NCOLS, C0, b, 0, fp, kp, None)),
                "scan": lambda i: ok(k_scan(kp, blocks, cp, None)),
                "scatter": lambda i: ok(k_scatter(pool(i).s.data, ld, N, NCOLS, C0, b, 0, fp, kp, dst.s.data, dst.ld, N, sp, -1, None)),
                "scatter_1_lane": lambda i: ok(k_scatter(pool(i).s.data, ld, N, NCOLS, C0, b, 0, fp, kp, dst.s.data, dst.ld, N, sp, 1, None)),
                "scatter_2_lanes": lambda i: ok(k_scatter(pool(i).s.data, ld, N, NCOLS, C0, b, 0, fp, kp, dst.s.data, dst.ld, N, sp, 2, None)),
                "pool_copy": lambda i: device.copy_block(dst, 0, 0, pool(i), 0, 0, N, NCOLS),
                "two_gathers": two_gathers,
            }
            if variant == 0:   # the other class-first kernel on the same table size: what moving the threshold would buy
                launches["first_global_atomics"] = lambda i: ok(k_first(pool(i).s.data, ld, N, C0, b, fp, 1, None))
            preset = lambda i: first.fill_(-1)  # noqa: E731
            t = timed_together(launches, {"first": preset, "first_global_atomics": preset})
            torch.cuda.synchronize()
            res = {"what": "lf1", "N": N, "b": b, "pool_bytes": N * 32, "buffers": rot, "first_variant": variant,
                   "rows_per_workgroup": rows, "survivors": idx[0][0]}
            for name, (med, lo, hi) in t.items():
                res[name + "_ms"] = round(med, 4)
                res[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            res["sum_of_launches_ms"] = round(sum(t[k][0] for k in ("first", "count", "scan", "scatter")), 4)
            res["composed_ms"] = round(sum(t[k][0] for k in ("first", "count", "scan", "count", "two_gathers")), 4)
            res["reduce_over_pool_copy"] = round(t["reduce"][0] / t["pool_copy"][0], 3)
            res["scatter_over_two_gathers"] = round(t["scatter"][0] / t["two_gathers"][0], 3)
            res["composed_over_sum_of_launches"] = round(res["composed_ms"] / res["sum_of_launches_ms"], 3)
            res["first_Grows_per_s"] = round(N / t["first"][0] / 1e6, 2)
            print(json.dumps(res), flush=True)
            del idx, first
            torch.cuda.empty_cache()
        if N == Ns[0]:
            # the route the entry replaces, once: download, numpy, upload
            import lf1_ref as lf
            b = 12 if not args.small else 3
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            words = pools[0].to_words()
            t1 = time.perf_counter()
            r = lf.lf1(words, NCOLS, C0, b)
            t2 = time.perf_counter()
            up = device.DMat.from_words(r.D, NCOLS)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            got = device.lf1_reduce(pools[0], C0, b)[0]
            same = bool(np.array_equal(got.to_words(), r.D))
            print(json.dumps({"what": "host route", "N": N, "b": b, "download_ms": round(1e3 * (t1 - t0), 2), "numpy_ms": round(1e3 * (t2 - t1), 2),
                              "upload_ms": round(1e3 * (t3 - t2), 2), "total_ms": round(1e3 * (t3 - t0), 2), "same_bits_as_the_device": same}),
                  flush=True)
            del up, got, words, r
        del tensors, pools, dst, src, counts
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
