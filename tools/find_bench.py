"""The row lookup through a hash table (gf2_find_rows_dev) on the device, next to a plain copy of the bytes of A and B and to the
route it replaces for A is B: gf2_unique_rows_dev, whose rep is the same array.

    python tools/find_bench.py [--reps 20] [--warmup 3] [--small]

Pools of 256 columns, N = 2^20 and 2^24 rows; for every N, in one run:
  self_distinct, self_half       gf2_find_rows_dev(P, P) on the full width, idx only: P random (no two rows are equal), and P with half
                                 its rows repeating an earlier row.  Before anything is timed idx is compared with the rep of
                                 gf2_unique_rows_dev on the same pool;
  unique_rep_distinct, _half     gf2_unique_rows_dev on the same pools, rep only (keep NULL, cap 0): the like-for-like route;
  self_half_mult                 self_half with mult and count;
  find_none, find_half, find_all NA = NB = N on the full width, idx, mult and count: no row, half the rows and every row of A occurs in B
                                 (B random; A another random pool, a gather of half B and half fresh rows, a permutation of B);
  find64_none, _half, _all       the same on the 64 columns [37, 101);
  build_only                     find_half with the first 256 rows of A alone: the fill and the build of the same table and one
                                 workgroup of the lookup.  lookup_ms = find_half - build_only;
  ab_copy                        gf2_copy_block_dev of the bytes of A and of B.

One process; every call is timed on its own with HIP events after --warmup calls, the figure is the median of --reps calls, and the
variants of a shape alternate call by call so that they see the same machine.  One JSON line per N; profiles/find_bench.txt keeps a
run."""
import argparse
import json
import os
import statistics
import sys

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

    ints = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")  # noqa: E731
    for N in ([1 << 12] if args.small else [1 << 20, 1 << 24]):
        B, fresh = device.DMat.random(N, NCOLS, 70), device.DMat.random(N, NCOLS, 71)
        gen = torch.Generator(device="cuda").manual_seed(90)
        perm = torch.randperm(N, generator=gen, device="cuda")
        draw = torch.randint(0, N // 2, (N,), generator=gen, device="cuda")
        # half the rows of `dup` repeat an earlier one: row i holds row src[i] of B, src a permutation below N / 2 and a draw above
        dup = device.gather_rows(B, torch.where(perm < N // 2, perm, draw).to(torch.int32).data_ptr(), D=device.DMat(N, NCOLS))[0]
        a_all = device.gather_rows(B, perm.to(torch.int32).data_ptr(), D=device.DMat(N, NCOLS))[0]
        # half of a_half's rows are rows of B, the others rows of `fresh`: B stacked on fresh, gathered
        both = device.stack(B, fresh)
        pick = torch.where(perm % 2 == 0, draw, N + perm).to(torch.int32)
        a_half = device.gather_rows(both, pick.data_ptr(), D=device.DMat(N, NCOLS))[0]
        del both
        a_first = device.DMat.wrap(a_half.s.data, 256, NCOLS, a_half.ld, keep=a_half)
        torch.cuda.synchronize()
        dst = device.DMat(N, NCOLS)
        idx, mult, rep, count, skip = ints(N), ints(N), ints(N), ints(4), device.SKIP
        ip, mp, rp, cp = idx.data_ptr(), mult.data_ptr(), rep.data_ptr(), count.data_ptr()
        res = {"what": "find", "N": N, "ncols": NCOLS, "pool_bytes": N * 32}
        # the like-for-like comparison first: the same array from both routes
        for name, P in (("distinct", B), ("half", dup)):
            device.find_rows(P, P, 0, NCOLS, idx=ip, mult=skip, count=cp)
            device.unique_rows(P, 0, NCOLS, keep=skip, cap=0, count=cp + 4, rep=rp)
            torch.cuda.synchronize()
            assert torch.equal(idx, rep), name
            res["classes_" + name] = int(count[1])
            assert int(count[0]) == N
        launches = {
            "self_distinct": lambda: device.find_rows(B, B, 0, NCOLS, idx=ip, mult=skip, count=skip),
            "unique_rep_distinct": lambda: device.unique_rows(B, 0, NCOLS, keep=skip, cap=0, count=cp, rep=rp),
            "self_half": lambda: device.find_rows(dup, dup, 0, NCOLS, idx=ip, mult=skip, count=skip),
            "unique_rep_half": lambda: device.unique_rows(dup, 0, NCOLS, keep=skip, cap=0, count=cp, rep=rp),
            "self_half_mult": lambda: device.find_rows(dup, dup, 0, NCOLS, idx=ip, mult=mp, count=cp),
            "find_none": lambda: device.find_rows(fresh, B, 0, NCOLS, idx=ip, mult=mp, count=cp),
            "find_half": lambda: device.find_rows(a_half, B, 0, NCOLS, idx=ip, mult=mp, count=cp),
            "find_all": lambda: device.find_rows(a_all, B, 0, NCOLS, idx=ip, mult=mp, count=cp),
            "find64_none": lambda: device.find_rows(fresh, B, C0, C0 + 64, idx=ip, mult=mp, count=cp),
            "find64_half": lambda: device.find_rows(a_half, B, C0, C0 + 64, idx=ip, mult=mp, count=cp),
            "find64_all": lambda: device.find_rows(a_all, B, C0, C0 + 64, idx=ip, mult=mp, count=cp),
            "build_only": lambda: device.find_rows(a_first, B, 0, NCOLS, idx=ip, mult=mp, count=cp),
            "ab_copy": lambda: (device.copy_block(dst, 0, 0, a_half, 0, 0, N, NCOLS), device.copy_block(dst, 0, 0, B, 0, 0, N, NCOLS)),
        }
        t = timed_together(launches)
        found = {}
        for name in ("find_none", "find_half", "find_all"):
            launches[name]()
            torch.cuda.synchronize()
            found[name] = int(count[0])
        assert found["find_none"] == 0 and found["find_all"] == N and N // 4 < found["find_half"] < 3 * N // 4, found
        plan = device.find_rows_plan(N, N, NCOLS, 0, NCOLS)
        res.update({"found": found, "slots": plan[1], "table_bytes": plan[3], "launches": plan[4]})
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
        res["lookup_ms"] = round(t["find_half"][0] - t["build_only"][0], 4)
        res["self_distinct_over_unique_rep"] = round(t["self_distinct"][0] / t["unique_rep_distinct"][0], 3)
        res["self_half_over_unique_rep"] = round(t["self_half"][0] / t["unique_rep_half"][0], 3)
        res["find_half_over_ab_copy"] = round(t["find_half"][0] / t["ab_copy"][0], 1)
        res["ab_copy_GBps"] = round(4 * N * 32 / t["ab_copy"][0] / 1e6, 1)
        print(json.dumps(res), flush=True)
        del B, fresh, dup, a_all, a_half, a_first, dst, idx, mult, rep, launches
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
