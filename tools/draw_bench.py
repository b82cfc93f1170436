"""The device draws (include/m4ri_hip_draw.h), each next to a plain copy of the same output bytes in the same run; Bernoulli also next
to gf2_dmat_fill_random on the same shape (the uniform fill, the nearest path the library had), the permutation next to the class
sort alone.

    python tools/draw_bench.py [--reps 20] [--warmup 3] [--small]

  bernoulli     2^26 x 1 and 2^20 x 256, thr = 0x20000000 (tau = 1/8, two Philox calls per word) and thr = 0x12345679 (sixteen);
                beside: gf2_copy_block_dev of the matrix, gf2_dmat_fill_random
  indices       2^26 draws below 2^20; beside: a copy of the array's bytes
  subsets       2^14 subsets of 512 out of 2^20; beside: a copy of the array's bytes
  permutation   n = 8192 and n = 2^20; beside: gf2_class_sort_dev of n rows by a 30-bit window (the four passes without the pair kernel)

One process; every launch is timed on its own with HIP events after --warmup launches, the figure is the median of --reps launches,
and the variants of a shape alternate launch by launch so that they see the same machine.  One JSON line per shape;
profiles/draw_bench.txt keeps a run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


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
                launch(i)
                b.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[name].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    def report(res, t, out_bytes, ratios):
        for name, (med, lo, hi) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            res[name + "_GBps_of_output"] = round(out_bytes / med / 1e6, 1)
        for a, b in ratios:
            res["%s_over_%s" % (a, b)] = round(t[a][0] / t[b][0], 3)
        print(json.dumps(res), flush=True)

    def int_array(count):
        """count device ints as a tensor and as the matrix that a plain copy moves"""
        rows = -(-count // 128)
        t = torch.zeros(rows * 128, dtype=torch.int32, device="cuda")
        return t, device.DMat.wrap(t.data_ptr(), rows, 4096, 64, keep=t)

    # ---- Bernoulli
    for nrows, ncols in ((1 << 12, 1), (1 << 10, 256)) if args.small else ((1 << 26, 1), (1 << 20, 256)):
        D, C = device.DMat(nrows, ncols), device.DMat(nrows, ncols)
        words = nrows * ((ncols + 63) // 64)
        launches = {
            "bernoulli_2_calls": lambda i: device.bernoulli(D, 0x20000000, 100 + i),
            "bernoulli_16_calls": lambda i: device.bernoulli(D, 0x12345679, 100 + i),
            "bernoulli_16_calls_accumulate": lambda i: device.bernoulli(D, 0x12345679, 100 + i, accumulate=True),
            "fill_random": lambda i: D.fill_random(100 + i),
            "copy": lambda i: device.copy_block(C, 0, 0, D, 0, 0, nrows, ncols),
        }
        t = timed_together(launches)
        res = {"what": "bernoulli", "nrows": nrows, "ncols": ncols, "ld": int(D.ld), "output_bytes": 8 * words,
               "philox_calls_per_word": [device.draw_plan("bernoulli", thr=thr)[0] for thr in (0x20000000, 0x12345679)]}
        for name in ("bernoulli_2_calls", "bernoulli_16_calls"):
            calls = 2 if "2_calls" in name else 16
            res[name + "_G_philox_calls_per_s"] = round(calls * words / t[name][0] / 1e6, 2)
        report(res, t, 8 * words, [("bernoulli_2_calls", "copy"), ("bernoulli_16_calls", "copy"), ("bernoulli_2_calls", "fill_random"),
                                   ("bernoulli_16_calls", "fill_random"), ("fill_random", "copy")])
        del D, C, launches
        L.gf2_trim()

    # ---- indices
    count, n = (1 << 16, 1 << 20) if args.small else (1 << 26, 1 << 20)
    ti, Mi = int_array(count)
    tc, Mc = int_array(count)
    t = timed_together({"indices": lambda i: device.draw_indices(count, n, 200 + i, out=ti.data_ptr()),
                        "copy": lambda i: device.copy_block(Mc, 0, 0, Mi, 0, 0, Mi.nrows, 4096)})
    report({"what": "indices", "count": count, "n": n, "output_bytes": 4 * count,
            "G_draws_per_s": round(count / t["indices"][0] / 1e6, 2)}, t, 4 * count, [("indices", "copy")])
    del ti, Mi, tc, Mc

    # ---- subsets
    batch, k, n = (1 << 8, 512, 1 << 20) if args.small else (1 << 14, 512, 1 << 20)
    ts, Ms = int_array(batch * k)
    tc, Mc = int_array(batch * k)
    unf = torch.zeros(4, dtype=torch.int32, device="cuda")
    t = timed_together({"subsets": lambda i: device.draw_subsets(batch, k, n, 300 + i, out=ts.data_ptr(), unfinished=unf.data_ptr()),
                        "copy": lambda i: device.copy_block(Mc, 0, 0, Ms, 0, 0, Ms.nrows, 4096)})
    plan = device.draw_plan("subsets", k, n)
    report({"what": "subsets", "batch": batch, "k": k, "n": n, "output_bytes": 4 * batch * k, "threads": plan[0], "lds_bytes": plan[1],
            "subsets_per_workgroup": plan[2], "unfinished": int(unf[0]), "M_subsets_per_s": round(batch / t["subsets"][0] / 1e3, 3)},
           t, 4 * batch * k, [("subsets", "copy")])
    del ts, Ms, tc, Mc

    # ---- permutation
    for n in (1 << 10,) if args.small else (8192, 1 << 20):
        tp, _ = int_array(n)
        to, _ = int_array(n)
        P = device.DMat.random(n, 64, 7)
        t = timed_together({"permutation": lambda i: device.draw_permutation(n, 400 + i, out=tp.data_ptr()),
                            "class_sort": lambda i: device.class_sort(P, 0, 30, order=to.data_ptr(), skeys=device.SKIP)})
        plan = device.draw_plan("permutation", n=n)
        report({"what": "permutation", "n": n, "output_bytes": 4 * n, "scratch_bytes": plan[0], "sort_passes": plan[1],
                "is_a_permutation": bool(torch.equal(torch.sort(tp[:n]).values, torch.arange(n, dtype=torch.int32, device="cuda")))},
               t, 4 * n, [("permutation", "class_sort")])
        del tp, to, P
    L.gf2_trim()


if __name__ == "__main__":
    main()
