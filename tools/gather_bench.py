"""Column and row gathers by device index arrays (gf2_gather_cols_dev, gf2_gather_rows_dev) next to the composed route through the
public pieces and next to a plain copy of the same bytes.

    python tools/gather_bench.py [--reps 20] [--warmup 3] [--small]

Column gather, each shape with a random permutation of the source's columns as index:
  (a) gf2_gather_cols_dev;
  (b) the composed route called through the public pieces: gf2_transpose_dev, gf2_gather_rows_dev, gf2_transpose_dev (what a caller
      could do before, and what the entry does where gf2_gather_cols_plan returns 1);
  (c) gf2_copy_block_dev of the whole matrix, aligned: the same bytes read and written once.
Shapes: 8192 x 8192, 65536 x 8192 and 65536 x the widest source the plan still gives to the fused kernel.  Row gather: 65536 x 65536
and 2^20 x 256, a random permutation of the rows, against (c).

One process; every launch is timed on its own with HIP events after --warmup launches of that shape, the figure is the median of --reps
launches, and the three variants of a shape alternate launch by launch so that they see the same machine.  Sources and destinations
rotate through three buffers each, so that from 65536 x 8192 (64 MiB a buffer) on no launch finds all of its operands in the 256 MiB
last-level cache; 8192 x 8192 (8 MiB) is a cache-resident shape and says so.  After the timing (a) is compared with (b) by
gf2_equal_dev.  One JSON line per shape; profiles/gather_bench.txt keeps a run.

The condition the plan has to meet: wherever it chooses the fused kernel, (a) is not slower than (b) in the same run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROT = 3


def widest_fused(device, nrows):
    lo, hi = 1, 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if device.gather_cols_plan(nrows, mid, mid)[0] == 0 else (lo, mid)
    return lo


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

    def ints(values):
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).cuda()

    def report(what, shape, nbytes, t, extra):
        out = {"what": what, "shape": shape, "bytes": nbytes}
        for k, (med, lo, hi) in t.items():
            out[k + "_ms"] = round(med, 4)
            out[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            out[k + "_TBps"] = round(nbytes / med / 1e9, 3)
        out.update(extra)
        print(json.dumps(out), flush=True)

    rng = np.random.default_rng(2024)
    big = 512 if args.small else 65536
    wide = widest_fused(device, big)
    col_shapes = [(big // 8, 8192 if not args.small else 640), (big, 8192 if not args.small else 640), (big, wide)]
    for rows, n in col_shapes:
        path = device.gather_cols_plan(rows, n, n)[0]
        src = [device.DMat.random(rows, n, 10 + i) for i in range(ROT)]
        dst = [device.DMat(rows, n) for _ in range(ROT)]
        dst_b = [device.DMat(rows, n) for _ in range(ROT)]
        st, gt = device.DMat(n, rows), device.DMat(n, rows)   # the composed route's intermediates, allocated once like stream scratch
        idx = ints(rng.permutation(n))

        def composed(i):
            device.transpose(src[i % ROT], D=st)
            device.gather_rows(st, idx.data_ptr(), D=gt)
            device.transpose(gt, D=dst_b[i % ROT])

        t = timed_together({
            "a_gather_cols": lambda i: device.gather_cols(src[i % ROT], idx.data_ptr(), D=dst[i % ROT]),
            "b_composed": composed,
            "c_copy": lambda i: device.copy_block(dst[(i + 1) % ROT], 0, 0, src[i % ROT], 0, 0, rows, n),
        })
        device.gather_cols(src[0], idx.data_ptr(), D=dst[0])
        st2 = device.transpose(src[0])
        device.gather_rows(st2, idx.data_ptr(), D=gt)
        device.transpose(gt, D=dst_b[0])
        same = device.equal(dst[0], dst_b[0])
        nbytes = 2 * rows * ((n + 63) // 64) * 8
        report("column gather", [rows, n, n], nbytes, t, {
            "plan": "fused" if path == 0 else "composed", "a_over_b": round(t["a_gather_cols"][0] / t["b_composed"][0], 3),
            "a_rate_over_copy": round(t["c_copy"][0] / t["a_gather_cols"][0], 3),
            "cache_resident": bool(3 * nbytes // 2 * ROT <= (256 << 20)), "same_bits": bool(same)})
        del src, dst, dst_b, st, gt, st2
        torch.cuda.empty_cache()

    row_shapes = [(big, big), ((1 << 20) if not args.small else 4096, 256)]
    for rows, n in row_shapes:
        src = [device.DMat.random(rows, n, 20 + i) for i in range(ROT)]
        dst = [device.DMat(rows, n) for _ in range(ROT)]
        perm = rng.permutation(rows)
        idx = ints(perm)
        t = timed_together({
            "gather_rows": lambda i: device.gather_rows(src[i % ROT], idx.data_ptr(), D=dst[i % ROT]),
            "c_copy": lambda i: device.copy_block(dst[(i + 1) % ROT], 0, 0, src[i % ROT], 0, 0, rows, n),
        })
        device.gather_rows(src[0], idx.data_ptr(), D=dst[0])
        inverse = ints(np.argsort(perm))
        back = device.gather_rows(dst[0], inverse.data_ptr(), D=dst[1])[0]
        same = device.equal(back, src[0])
        nbytes = 2 * rows * ((n + 63) // 64) * 8
        report("row gather", [rows, rows, n], nbytes, t, {
            "rate_over_copy": round(t["c_copy"][0] / t["gather_rows"][0], 3), "same_bits": bool(same)})
        del src, dst, back
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
