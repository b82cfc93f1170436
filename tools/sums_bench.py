"""All XORs of p rows of a matrix in rank order (gf2_subset_sums_dev), next to a plain copy of the output bytes, the route it replaces
(index arrays that are on the device already, then p passes of gf2_gather_rows_dev) and, for the shapes that a host can turn around
in seconds, the full host route (download S, numpy, upload the list).

    python tools/sums_bench.py [--reps 10] [--warmup 2] [--small]

S has 256 columns of random bits and base is one more such row; weights over the columns [70, 256).  Shapes: p = 2 with n = 4096
(8.4 million sums, about 2^23) and n = 11585 (67.1 million, about 2^26); p = 3 with n = 738 and p = 4 with n = 203, both about 2^26;
and p = 2 with n = 64 (2016 sums), where the launch is all there is.  For every shape, in one run:
  sums          gf2_subset_sums_dev with the rows, idx and wt;
  sums_rows     the rows alone (idx and wt NULL);
  sums_wt       rows not stored: the weights alone (D->data NULL);
  sums_idx_wt   rows not stored: idx and wt;
  sums_global   where the plan copies S into LDS: the same launch as sums_rows with S read from global memory instead, singly through
                the library's launcher (csrc/sums/gf2_sums.h); sums_lds is then sums_rows through that launcher;
  gathers       p passes of gf2_gather_rows_dev over the list, the first storing and the others accumulating, from p index arrays
                made beforehand (by gf2_unrank_subsets_dev and a column split): the route without this entry.  base is left out of it;
  copy          gf2_copy_block_dev of the rows that sums_rows wrote: the output bytes once read and once written;
  fill          gf2_dmat_fill_random of the same rows: the output bytes written only;
  host_route    (p = 2 with n = 4096 and n = 64 only) S downloaded, the list made in numpy, uploaded; one run, a host clock.

One process; every device variant is timed on its own with HIP events after --warmup runs, the figure is the median of --reps runs,
and the variants of a shape alternate run by run so that they see the same machine.  The rows of `sums` are compared with the rows
that the gathers made, on the device.  One JSON line per shape; profiles/sums_bench.txt keeps a run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS, WC0, WC1 = 256, 70, 256
LD = NCOLS // 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    k_sums = L.gf2k_subset_sums
    k_sums.restype, k_sums.argtypes = I, [P, LL, I, P, I, I, LL, LL, P, LL, P, P, I, I, I, P]

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
    shapes = [(2, 64, True), (2, 300, True), (3, 60, False), (4, 30, False)] if args.small else \
        [(2, 64, True), (2, 4096, True), (2, 11585, False), (3, 738, False), (4, 203, False)]
    for p, n, host in shapes:
        count = device.subset_count(n, p)
        plan = device.subset_sums_plan(n, NCOLS, p, count)
        ts = torch.empty((n, LD), dtype=torch.int64, device="cuda")
        tb = torch.empty((1, LD), dtype=torch.int64, device="cuda")
        td, td2 = (torch.empty((count, LD), dtype=torch.int64, device="cuda") for _ in range(2))
        S, B = device.DMat.from_torch(ts, NCOLS), device.DMat.from_torch(tb, NCOLS)
        D, D2 = device.DMat.from_torch(td, NCOLS), device.DMat.from_torch(td2, NCOLS)
        S.fill_random(40 + n)
        B.fill_random(140 + n)
        none = device.DMat.wrap(None, count, NCOLS, LD)
        idx, wt = ints(count * p), ints(count)
        # beforehand: the p index arrays of the route, c_i of every rank, each contiguous
        ranks = torch.arange(count, dtype=torch.int32, device="cuda")
        device.unrank_subsets(ranks.data_ptr(), count, p, n, idx=idx.data_ptr(), bad=device.SKIP)
        torch.cuda.synchronize()
        cols = [idx.view(count, p)[:, i].contiguous() for i in range(p)]
        del ranks

        def sums(Dm, with_idx, with_wt, base=B):
            device.subset_sums(S, p, base=base, D=Dm, idx=idx.data_ptr() if with_idx else device.SKIP, wt=wt.data_ptr() if with_wt else device.SKIP,
                               wcols=(WC0, WC1))

        def unstored(with_idx):
            rc = L.gf2_subset_sums_dev(ctypes.byref(none.s), ctypes.byref(S.s), ctypes.byref(B.s), p, 0, idx.data_ptr() if with_idx else None,
                                       wt.data_ptr(), WC0, WC1, None)
            device._lib.check(rc, "gf2_subset_sums_dev")

        def launcher(global_s):
            ok(k_sums(S.s.data, S.ld, n, B.s.data, NCOLS, p, 0, count, D.s.data, D.ld, None, None, WC0, WC1, global_s, None))

        def gathers():
            for i in range(p):
                device.gather_rows(S, cols[i].data_ptr(), D=D2, accumulate=i > 0)

        launches = {
            "sums": lambda: sums(D, True, True),
            "sums_rows": lambda: sums(D, False, False),
            "sums_wt": lambda: unstored(False),
            "sums_idx_wt": lambda: unstored(True),
            "gathers": gathers,
            "copy": lambda: device.copy_block(D2, 0, 0, D, 0, 0, count, NCOLS),
            "fill": lambda: D2.fill_random(7),
        }
        if plan[0] < 4:
            launches["sums_lds"] = lambda: launcher(0)
            launches["sums_global"] = lambda: launcher(1)
        t = timed_together(launches)
        # the same rows by both routes (base left out of both)
        sums(D, False, False, base=None)
        gathers()
        torch.cuda.synchronize()
        same = bool(torch.equal(td, td2))
        res = {"what": "subset_sums", "p": p, "n": n, "ncols": NCOLS, "sums": count, "output_bytes": count * 8 * LD, "kernel_id": plan[0],
               "ranks_per_workgroup": plan[2], "lanes_per_row": plan[3], "lds_bytes": plan[4], "workgroups": plan[5],
               "rows_equal_the_gathers": same}
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
        out_bytes = count * 8 * LD
        res["sums_rows_GBps_written"] = round(out_bytes / t["sums_rows"][0] / 1e6, 1)
        res["sums_GBps_written"] = round((out_bytes + 4 * (p + 1) * count) / t["sums"][0] / 1e6, 1)
        res["copy_GBps_read_plus_written"] = round(2 * out_bytes / t["copy"][0] / 1e6, 1)
        res["fill_GBps_written"] = round(out_bytes / t["fill"][0] / 1e6, 1)
        res["sums_rows_over_copy"] = round(t["sums_rows"][0] / t["copy"][0], 3)
        res["sums_over_copy"] = round(t["sums"][0] / t["copy"][0], 3)
        res["sums_rows_over_fill"] = round(t["sums_rows"][0] / t["fill"][0], 3)
        res["gathers_over_sums_rows"] = round(t["gathers"][0] / t["sums_rows"][0], 3)
        res["sums_wt_over_sums_rows"] = round(t["sums_wt"][0] / t["sums_rows"][0], 3)
        if "sums_global" in t:
            res["sums_global_over_sums_lds"] = round(t["sums_global"][0] / t["sums_lds"][0], 3)
        if host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = S.to_words()
            c2 = np.repeat(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))        # p = 2 in rank order: c_2, and c_1 = 0 .. c_2 - 1
            c1 = np.arange(count, dtype=np.int64) - c2 * (c2 - 1) // 2
            rows = w[c1] ^ w[c2]
            t1 = time.perf_counter()
            H = device.DMat.from_words(rows, NCOLS)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res["host_route_ms"] = round(1e3 * (t2 - t0), 2)
            res["host_route_numpy_ms"] = round(1e3 * (t1 - t0), 2)
            res["host_route_equals"] = bool(device.equal(H, D))
            res["host_route_over_sums_rows"] = round(1e3 * (t2 - t0) / t["sums_rows"][0], 1)
            del H, rows, c1, c2, w
        print(json.dumps(res), flush=True)
        del ts, tb, td, td2, S, B, D, D2, idx, wt, cols, launches
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
