"""The join of two pools on a column range of any width (gf2_join_rows_dev) and the grouping by class (gf2_group_rows_dev) on the
device, next to a plain copy of the bytes of A, B and D, to the sort-merge join on a window (gf2_join_dev) where that one applies, and
to the row sort (gf2_sort_rows_dev) that the grouping stands in for.

    python tools/join_rows_bench.py [--log2n 20] [--reps 10] [--warmup 2] [--small] [--host]

Pools of 256 columns, NA = NB = N = 2^log2n rows (the recorded run: 20 and 24, one process each, each under its own timeout).  A and B
are N draws each, with replacement, from one dictionary of N random rows, so the whole rows of A and B meet in about N pairs; a narrow
range adds the chance collisions of its width (N^2 / 2^w), which the printed counts show.  In one run:
  join24 .. join256          gf2_join_rows_dev on the columns [0, w), w = 24, 30, 48, 64, 128, 256: D, ia, ib and wt (the ones on the
                             last 64 columns) at a capacity of exactly the count, which a count-only call gave beforehand;
  count64                    the count-only call on 64 columns;
  window24, window30         gf2_join_dev on the same 24 and 30 columns at the same capacity: the sort-merge route, which is allowed
                             to win there.  Before anything is timed its pairs, ordered by (ia, ib), are compared with join24's;
  group64, group256          gf2_group_rows_dev of B, order only;
  sort64, sort256            gf2_sort_rows_dev of B on the same ranges, order only;
  abd_copy                   gf2_copy_block_dev of the bytes of A, of B and of a D of the 64-column count.
--host (2^20 only): once, download of A and B, the join on 64 columns in numpy (sort, searchsorted, XOR), upload of D.

One process; every call is timed on its own with HIP events after --warmup calls, the figure is the median of --reps calls, and the
variants alternate call by call so that they see the same machine.  One JSON line; profiles/join_rows_bench.txt keeps a run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS = 256
WIDTHS = (24, 30, 48, 64, 128, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not rates)")
    ap.add_argument("--host", action="store_true", help="also the host route (download, numpy, upload), once")
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
                launch()
                b.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[name].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    N = 1 << (12 if args.small else args.log2n)
    ints = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")  # noqa: E731
    dictionary = device.DMat.random(N, NCOLS, 80)
    gen = torch.Generator(device="cuda").manual_seed(91)
    draws = [torch.randint(0, N, (N,), generator=gen, device="cuda").to(torch.int32) for _ in range(2)]
    A, B = (device.gather_rows(dictionary, d.data_ptr(), D=device.DMat(N, NCOLS))[0] for d in draws)
    torch.cuda.synchronize()
    del dictionary
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    cp, skip = count.data_ptr(), device.SKIP
    none = device.DMat.wrap(None, 0, NCOLS, A.ld)
    counts = {}
    for w in WIDTHS:                                         # the count-only calls: the capacities
        device.join_rows(A, B, 0, w, D=none, count=cp, ia=skip, ib=skip, wt=skip)
        torch.cuda.synchronize()
        counts[w] = int(count[0])
    cap = max(counts.values())
    assert cap < 1 << 31, counts
    D, dst = device.DMat(cap, NCOLS), device.DMat(cap, NCOLS)
    ia, ib, wt, ia2, ib2, order = ints(cap), ints(cap), ints(cap), ints(cap), ints(cap), ints(N)
    view = lambda n: device.DMat.wrap(D.s.data, n, NCOLS, D.ld, keep=D)  # noqa: E731
    res = {"what": "join_rows", "N": N, "ncols": NCOLS, "pool_bytes": N * 32, "pairs": counts}
    # the same pairs from both routes at 24 bits, ordered by (ia, ib)
    device.join_rows(A, B, 0, 24, D=view(counts[24]), count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(), wt=skip)
    device.join(A, B, 0, 24, D=view(counts[24]), count=cp + 8, ia=ia2.data_ptr(), ib=ib2.data_ptr(), wt=skip)
    torch.cuda.synchronize()
    n24 = counts[24]
    assert int(count[1]) == n24
    by = torch.argsort((ia2[:n24].to(torch.int64) << 32) | ib2[:n24].to(torch.int64))
    assert torch.equal(ia2[:n24][by], ia[:n24]) and torch.equal(ib2[:n24][by], ib[:n24])
    del by
    join = lambda w: lambda: device.join_rows(A, B, 0, w, D=view(counts[w]), count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(),  # noqa: E731
                                              wt=wt.data_ptr(), wcols=(NCOLS - 64, NCOLS))
    window = lambda w: lambda: device.join(A, B, 0, w, D=view(counts[w]), count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(),  # noqa: E731
                                           wt=wt.data_ptr(), wcols=(NCOLS - 64, NCOLS))
    launches = {"join%d" % w: join(w) for w in WIDTHS}
    launches.update({
        "count64": lambda: device.join_rows(A, B, 0, 64, D=none, count=cp, ia=skip, ib=skip, wt=skip),
        "window24": window(24),
        "window30": window(30),
        "group64": lambda: device.group_rows(B, 0, 64, order=order.data_ptr(), head=skip),
        "sort64": lambda: device.sort_rows(B, 0, 64, order=order.data_ptr(), head=skip),
        "group256": lambda: device.group_rows(B, 0, 256, order=order.data_ptr(), head=skip),
        "sort256": lambda: device.sort_rows(B, 0, 256, order=order.data_ptr(), head=skip),
        "abd_copy": lambda: (device.copy_block(dst, 0, 0, A, 0, 0, N, NCOLS), device.copy_block(dst, 0, 0, B, 0, 0, N, NCOLS),
                             device.copy_block(dst, 0, 0, D, 0, 0, counts[64], NCOLS)),
    })
    t = timed_together(launches)
    plan = device.join_rows_plan(N, N, NCOLS, 0, 64)
    res.update({"passes": plan[0], "slots": plan[1], "group_launches": plan[3], "join_launches": plan[4], "join_scratch_bytes": plan[8]})
    for name, (med, lo_, hi_) in t.items():
        res[name + "_ms"] = round(med, 4)
        res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
    res["join24_over_window24"] = round(t["join24"][0] / t["window24"][0], 3)
    res["join30_over_window30"] = round(t["join30"][0] / t["window30"][0], 3)
    res["join64_over_abd_copy"] = round(t["join64"][0] / t["abd_copy"][0], 1)
    res["group64_over_sort64"] = round(t["group64"][0] / t["sort64"][0], 3)
    res["group256_over_sort256"] = round(t["group256"][0] / t["sort256"][0], 3)
    res["abd_copy_GBps"] = round(2 * (2 * N + counts[64]) * 32 / t["abd_copy"][0] / 1e6, 1)
    if args.host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = A.to_words(), B.to_words()
        o = np.argsort(b[:, 0], kind="stable")
        keys = b[o, 0]
        lo, hi = np.searchsorted(keys, a[:, 0], "left"), np.searchsorted(keys, a[:, 0], "right")
        rows_a = np.repeat(np.arange(N), hi - lo)
        first = np.repeat(lo - np.r_[0, np.cumsum(hi - lo)[:-1]], hi - lo)
        rows_b = o[first + np.arange(len(rows_a))]
        device.DMat.from_words(a[rows_a] ^ b[rows_b], NCOLS)
        torch.cuda.synchronize()
        res["host_route64_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        assert len(rows_a) == counts[64]
    print(json.dumps(res), flush=True)
    L.gf2_trim()


if __name__ == "__main__":
    main()
