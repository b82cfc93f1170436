"""The join of two pools on a window with the weights of the XORs (gf2_join_dev), next to a plain copy of the bytes of A, B and D, an
LF2 round of the concatenated pool, and the LF2 pair scatter at an equal output count.

    python tools/join_bench.py [--reps 10] [--warmup 2] [--small]

Pools of 256 columns of random bits, window c0 = 37, NA = NB = m * 2^b rows for b = 18, 22, 24 and m = 1, 4; the expected count is
NA NB / 2^b = m^2 2^b, the capacity 1.2 times that; weights over the columns [70, 256).  For every shape, in one run:
  join          gf2_join_dev: the two sorts, count, scan, scatter with ia, ib and wt;
  join_count    the count-only call (D->nrows == 0): the two sorts, count, scan;
  sort_a, sort_b   gf2_class_sort_dev of A and of B alone;
  count         the count launches singly through the library's launcher (csrc/join/gf2_join.h), on sorted keys made beforehand;
  scatter       the scatter launch singly, with ia, ib and wt; scatter_rows: the same without the three int arrays;
  lf2_scatter   the LF2 pair scatter (csrc/lf2/gf2_lf2.h) of the concatenated pool [A ; B] with lo and hi, its capacity cut to the
                join's output count: the same number of rows written;
  lf2_concat    gf2_lf2_reduce_dev of the concatenated pool at the join's capacity: the route without this entry.  It also makes every
                pair inside A and inside B, and fills the capacity with them;
  copy          gf2_copy_block_dev of the bytes of A, of B and of the rows of D that the join wrote, three launches.

One process; every variant is timed on its own with HIP events after --warmup runs, the figure is the median of --reps runs, and the
variants of a shape alternate run by run so that they see the same machine.  The pools do not rotate: at b = 18 the operands fit the
last-level cache.  One JSON line per shape; profiles/join_bench.txt keeps a run."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS, C0, WC0, WC1 = 256, 37, 70, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not rates)")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from m4ri_rust_amd import device
    device.require_gpu()
    L = device._lib.lib()
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    k_count, k_scatter, k_lf2_count, k_lf2_scatter = L.gf2k_join_count, L.gf2k_join_scatter, L.gf2k_lf2_pair_count, L.gf2k_lf2_pair_scatter
    for fn, argtypes in ((k_count, [P, I, P, I, P, P, P]),
                         (k_scatter, [P, LL, I, P, LL, I, I, P, P, P, P, P, P, LL, I, P, P, P, I, I, I, P]),
                         (k_lf2_count, [P, I, P, P, P]), (k_lf2_scatter, [P, LL, I, I, P, P, P, P, LL, I, P, P, I, P])):
        fn.restype, fn.argtypes = I, argtypes

    def ok(rc):
        assert rc == 0, "a launcher returned hipError %d" % rc

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
    ld = NCOLS // 64
    shapes = [(8, 1), (8, 4)] if args.small else [(b, m) for b in (18, 22, 24) for m in (1, 4)]
    for b, m in shapes:
        N = m << b
        expected = m * m << b
        cap = int(1.2 * expected)
        ta, tb = (torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(2))
        tab = torch.empty((2 * N, ld), dtype=torch.int64, device="cuda")
        A, B, AB = device.DMat.from_torch(ta, NCOLS), device.DMat.from_torch(tb, NCOLS), device.DMat.from_torch(tab, NCOLS)
        A.fill_random(40 + b)
        B.fill_random(140 + b)
        device.stack(A, B, C=AB)
        plan = device.join_plan(N, N, NCOLS, b)
        passes, R, lanes, S, runs = plan[0], plan[2], plan[3], plan[4], plan[7]
        lf2_runs = -(-2 * N // device.lf2_plan(2 * N, NCOLS, b)[5])
        D, D2, A2, B2 = device.DMat(cap, NCOLS), device.DMat(cap, NCOLS), device.DMat(N, NCOLS), device.DMat(N, NCOLS)
        ia, ib, wt = ints(cap), ints(cap), ints(cap)
        count = torch.zeros(2, dtype=torch.int64, device="cuda")
        cp = count.data_ptr()
        # beforehand: the sorted orders and keys, the run offsets of the join and of the LF2 round of [A ; B]
        oa, ka, ob, kb, oab, kab = ints(N), ints(N), ints(N), ints(N), ints(2 * N), ints(2 * N)
        sums, lf2_sums = (torch.zeros(r, dtype=torch.int64, device="cuda") for r in (runs, lf2_runs))
        device.class_sort(A, C0, b, order=oa.data_ptr(), skeys=ka.data_ptr())
        device.class_sort(B, C0, b, order=ob.data_ptr(), skeys=kb.data_ptr())
        device.class_sort(AB, C0, b, order=oab.data_ptr(), skeys=kab.data_ptr())
        ok(k_lf2_count(kab.data_ptr(), 2 * N, lf2_sums.data_ptr(), cp, None))
        torch.cuda.synchronize()
        lf2_pairs = int(count[0])
        ok(k_count(ka.data_ptr(), N, kb.data_ptr(), N, sums.data_ptr(), cp, None))
        torch.cuda.synchronize()
        n_out = int(count[0])
        written = min(n_out, cap)
        order_tmp, skeys_tmp, sums_tmp = ints(N), ints(N), torch.zeros(runs, dtype=torch.int64, device="cuda")
        Dn, D2n = (device.DMat.wrap(x.s.data, written, NCOLS, x.ld, keep=x) for x in (D, D2))

        def scatter(with_ints):
            p = (ia.data_ptr(), ib.data_ptr(), wt.data_ptr()) if with_ints else (None, None, None)
            ok(k_scatter(A.s.data, ld, N, B.s.data, ld, N, NCOLS, oa.data_ptr(), ka.data_ptr(), ob.data_ptr(), kb.data_ptr(), sums.data_ptr(),
                         D.s.data, D.ld, cap, p[0], p[1], p[2], WC0, WC1, -1, None))

        def copies():
            device.copy_block(A2, 0, 0, A, 0, 0, N, NCOLS)
            device.copy_block(B2, 0, 0, B, 0, 0, N, NCOLS)
            device.copy_block(D2n, 0, 0, Dn, 0, 0, written, NCOLS)

        none = device.DMat.wrap(None, 0, NCOLS, ld)
        launches = {
            "join": lambda: device.join(A, B, C0, b, D=D, count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(), wt=wt.data_ptr(), wcols=(WC0, WC1)),
            "join_count": lambda: device.join(A, B, C0, b, D=none, count=cp, ia=device.SKIP, ib=device.SKIP, wt=device.SKIP),
            "sort_a": lambda: device.class_sort(A, C0, b, order=order_tmp.data_ptr(), skeys=skeys_tmp.data_ptr()),
            "sort_b": lambda: device.class_sort(B, C0, b, order=order_tmp.data_ptr(), skeys=skeys_tmp.data_ptr()),
            "count": lambda: ok(k_count(ka.data_ptr(), N, kb.data_ptr(), N, sums_tmp.data_ptr(), cp, None)),
            "scatter": lambda: scatter(True),
            "scatter_rows": lambda: scatter(False),
            "lf2_scatter": lambda: ok(k_lf2_scatter(AB.s.data, ld, 2 * N, NCOLS, oab.data_ptr(), kab.data_ptr(), lf2_sums.data_ptr(), D2.s.data, D2.ld,
                                                    written, ia.data_ptr(), ib.data_ptr(), -1, None)),
            "lf2_concat": lambda: device.lf2_reduce(AB, C0, b, D=D2, count=cp, lo=ia.data_ptr(), hi=ib.data_ptr()),
            "copy": copies,
        }
        t = timed_together(launches)
        torch.cuda.synchronize()
        res = {"what": "join", "NA": N, "NB": N, "b": b, "pool_bytes_each": N * 32, "expected": expected, "capacity": cap, "pairs": n_out,
               "lf2_pairs_of_the_concatenated_pool": lf2_pairs, "passes": passes, "run_rows": R, "span_keys": S, "lanes_per_row": lanes,
               "lds_bytes": plan[5], "scratch_bytes": plan[6]}
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
        copy_bytes = 2 * (2 * N + written) * 32          # read and written
        res["copy_bytes"] = copy_bytes
        res["copy_GBps"] = round(copy_bytes / t["copy"][0] / 1e6, 1)
        res["join_over_copy"] = round(t["join"][0] / t["copy"][0], 3)
        res["join_over_lf2_concat"] = round(t["join"][0] / t["lf2_concat"][0], 3)
        res["scatter_over_lf2_scatter"] = round(t["scatter"][0] / t["lf2_scatter"][0], 3)
        res["scatter_rows_over_lf2_scatter"] = round(t["scatter_rows"][0] / t["lf2_scatter"][0], 3)
        res["sum_of_parts_ms"] = round(t["sort_a"][0] + t["sort_b"][0] + t["count"][0] + t["scatter"][0], 4)
        # the floor: passes x 16 bytes per row of the two sorts, two rows read and one written per output, 12 bytes of ints per output
        floor_bytes = passes * 16 * 2 * N + (3 * 32 + 12) * written
        res["floor_bytes"] = floor_bytes
        res["join_GBps_of_floor_bytes"] = round(floor_bytes / t["join"][0] / 1e6, 1)
        print(json.dumps(res), flush=True)
        del ta, tb, tab, A, B, AB, D, D2, Dn, D2n, A2, B2, ia, ib, wt, oa, ka, ob, kb, oab, kab, sums, lf2_sums, order_tmp, skeys_tmp, sums_tmp, launches
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
