"""The row sort on a column range (gf2_sort_rows_dev) and the duplicate removal (gf2_unique_rows_dev) on the device, next to a plain
copy of the pool's bytes, the class sort on the same 24-bit window, and the host route that they replace.

    python tools/unique_bench.py [--reps 20] [--warmup 3] [--small] [--no-host]

Pools of 256 columns, N = 2^20 and 2^24 rows; for every N, in one run:
  sort_24, sort_64, sort_256   gf2_sort_rows_dev on the columns [37, 61), [37, 101) and [0, 256) of pools of random bits, order only;
  sort_256_head                the same with head: three launches more;
  unique_distinct              gf2_unique_rows_dev on the full width of the same pools (no two rows are equal), keep with cap = N, no rep;
  unique_half                  the same on pools in which half the rows repeat an earlier row: N / 2 distinct rows, scattered;
  unique_half_rep              ... with rep;
  class_sort_24                gf2_class_sort_dev on the window [37, 61) of the same pools, order only: the same three passes, the first
                               of which reads its keys from the rows where sort_24 has a rekey launch write pairs first;
  pool_copy                    gf2_copy_block_dev of the pool's bytes.
Once per N the host route: download, numpy.unique(axis=0, return_index=True) and the sort of the first indices, upload of the kept
rows; its kept rows must be the device's.

One process; every call is timed on its own with HIP events after --warmup calls, the figure is the median of --reps calls, and the
variants of a shape alternate call by call so that they see the same machine.  The pools rotate through as many buffers as it takes
to hold 768 MiB (at least three).  One JSON line per shape; profiles/unique_bench.txt keeps a run."""
import argparse
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
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from m4ri_rust_amd import device
    device.require_gpu()
    L = device._lib.lib()

    def timed_together(launches):
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

    ints = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")  # noqa: E731
    ld = NCOLS // 64
    for N in ([1 << 12] if args.small else [1 << 20, 1 << 24]):
        rot = 3 if args.small else max(3, -(-(768 << 20) // (N * 32)))
        tensors = [torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(rot)]
        pools = [device.DMat.from_torch(t, NCOLS) for t in tensors]
        for i, p in enumerate(pools):
            p.fill_random(70 + i)
        # half the rows repeat an earlier one: row i holds row src[i] of a random pool, src a permutation below N / 2 and a draw above
        half = [device.DMat(N, NCOLS) for _ in range(min(rot, 3))]
        for i, h in enumerate(half):
            gen = torch.Generator(device="cuda").manual_seed(90 + i)
            perm = torch.randperm(N, generator=gen, device="cuda")
            draw = torch.randint(0, N // 2, (N,), generator=gen, device="cuda")
            src = torch.where(perm < N // 2, perm, draw).to(torch.int32)
            device.gather_rows(pools[i], src.data_ptr(), D=h)
        torch.cuda.synchronize()
        dst = device.DMat(N, NCOLS)
        order, head, skip, keep, rep = ints(N), ints(N), device.SKIP, ints(N), ints(N)
        count = ints(4)
        op, hp, kp, cp, rp = order.data_ptr(), head.data_ptr(), keep.data_ptr(), count.data_ptr(), rep.data_ptr()
        pool = lambda i: pools[i % rot]  # noqa: E731
        dup = lambda i: half[i % len(half)]  # noqa: E731
        launches = {
            "sort_24": lambda i: device.sort_rows(pool(i), C0, C0 + 24, order=op, head=skip),
            "sort_64": lambda i: device.sort_rows(pool(i), C0, C0 + 64, order=op, head=skip),
            "sort_256": lambda i: device.sort_rows(pool(i), 0, NCOLS, order=op, head=skip),
            "sort_256_head": lambda i: device.sort_rows(pool(i), 0, NCOLS, order=op, head=hp),
            "unique_distinct": lambda i: device.unique_rows(pool(i), 0, NCOLS, keep=kp, cap=N, count=cp, rep=skip),
            "unique_half": lambda i: device.unique_rows(dup(i), 0, NCOLS, keep=kp, cap=N, count=cp, rep=skip),
            "unique_half_rep": lambda i: device.unique_rows(dup(i), 0, NCOLS, keep=kp, cap=N, count=cp, rep=rp),
            "class_sort_24": lambda i: device.class_sort(pool(i), C0, 24, order=op, skeys=skip),
            "pool_copy": lambda i: device.copy_block(dst, 0, 0, pool(i), 0, 0, N, NCOLS),
        }
        t = timed_together(launches)
        device.unique_rows(pools[0], 0, NCOLS, keep=kp, cap=N, count=cp, rep=skip)
        torch.cuda.synchronize()
        distinct = int(count[0])
        device.unique_rows(half[0], 0, NCOLS, keep=kp, cap=N, count=cp, rep=skip)
        torch.cuda.synchronize()
        kept = int(count[0])
        plans = {w: device.sort_rows_plan(N, NCOLS, c0, c0 + w) for w, c0 in ((24, C0), (64, C0), (256, 0))}
        res = {"what": "unique", "N": N, "ncols": NCOLS, "pool_bytes": N * 32, "buffers": rot, "distinct_rows_of_the_random_pool": distinct,
               "distinct_rows_of_the_half_pool": kept, "passes": {w: p[0] for w, p in plans.items()},
               "windows": {w: p[1] for w, p in plans.items()}, "sort_launches": {w: p[4] for w, p in plans.items()},
               "unique_launches": plans[256][5], "sort_scratch_bytes": plans[256][6], "unique_scratch_bytes": plans[256][7]}
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
        res["sort_24_minus_class_sort_24_ms"] = round(t["sort_24"][0] - t["class_sort_24"][0], 4)
        res["sort_256_ms_per_pass"] = round(t["sort_256"][0] / plans[256][0], 4)
        res["heads_ms"] = round(t["sort_256_head"][0] - t["sort_256"][0], 4)
        res["unique_half_minus_sort_256_ms"] = round(t["unique_half"][0] - t["sort_256"][0], 4)
        res["unique_half_over_pool_copy"] = round(t["unique_half"][0] / t["pool_copy"][0], 1)
        res["pool_copy_GBps"] = round(2 * N * 32 / t["pool_copy"][0] / 1e6, 1)
        # the floor of the sort: 16 bytes per row and pass (a pair read, a pair written), 8 per row and window of the rekey's pairs
        floor_bytes = 16 * N * plans[256][0] + 8 * N * plans[256][1]
        res["sort_256_GBps_of_floor_bytes"] = round(floor_bytes / t["sort_256"][0] / 1e6, 1)
        print(json.dumps(res), flush=True)
        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            words = half[0].to_words()
            t1 = time.perf_counter()
            _, first = np.unique(words, axis=0, return_index=True)
            first.sort()
            t2 = time.perf_counter()
            up = device.DMat.from_words(words[first], NCOLS)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            same = bool(np.array_equal(keep.cpu().numpy()[:kept], first))
            print(json.dumps({"what": "host route", "N": N, "kept": int(len(first)), "download_ms": round(1e3 * (t1 - t0), 2),
                              "numpy_unique_ms": round(1e3 * (t2 - t1), 2), "upload_ms": round(1e3 * (t3 - t2), 2),
                              "total_ms": round(1e3 * (t3 - t0), 2), "same_kept_rows_as_the_device": same}), flush=True)
            del up, words, first
        del tensors, pools, half, dst, order, head, keep, rep, launches
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
