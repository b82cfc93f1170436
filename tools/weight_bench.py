"""Hamming weights on the device (gf2_row_weights_dev, gf2_col_weights_dev, gf2_count_ones_dev, gf2_select_weights_dev) next to a plain
copy of the same bytes and, for the column weights, next to the composed route through shipped entries.

    python tools/weight_bench.py [--reps 20] [--warmup 3] [--small]

Shapes: 65536 x 65536 (512 MiB) and 2^20 x 256 (32 MiB, the LPN shape).  Per shape, in one run:
  rows    gf2_row_weights_dev;
  cols    gf2_col_weights_dev;
  b_composed   gf2_transpose_dev, then gf2_row_weights_dev of the result (what a caller could do for column weights before);
  total   gf2_count_ones_dev (65536 x 65536 only);
  c_copy  gf2_copy_block_dev of the whole matrix, aligned: the operand's bytes read once and written once.  The weight kernels only
          read, so at or below the copy's time is the expectation.
Select: 2^20 weights with about 0.1 % matches, next to a device-to-device copy of the weights.

One process; every launch is timed on its own with HIP events after --warmup launches of that shape, the figure is the median of --reps
launches, and the variants of a shape alternate launch by launch so that they see the same machine.  The operands rotate through as
many buffers as it takes to hold 768 MiB (at least three), so that no launch finds its operand in the 256 MiB last-level cache.  After
the timing the column weights are compared with the composed route's and the three sums with each other.  One JSON line per shape;
profiles/weight_bench.txt keeps a run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

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

    def report(what, shape, nbytes, t, extra):
        out = {"what": what, "shape": shape, "operand_bytes": nbytes}
        for k, (med, lo, hi) in t.items():
            out[k + "_ms"] = round(med, 4)
            out[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            if k != "c_copy":
                out[k + "_read_TBps"] = round(nbytes / med / 1e9, 3)
                out[k + "_over_copy"] = round(med / t["c_copy"][0], 3)
        out.update(extra)
        print(json.dumps(out), flush=True)

    shapes = [(512, 4096), (4096, 256)] if args.small else [(65536, 65536), (1 << 20, 256)]
    for rows, n in shapes:
        nbytes = rows * ((n + 63) // 64) * 8
        rot = max(3, -(-(768 << 20) // nbytes)) if not args.small else 3
        src = [device.DMat.random(rows, n, 10 + i) for i in range(rot)]
        dst = [device.DMat(rows, n) for _ in range(3)]
        tr = device.DMat(n, rows)   # the composed route's intermediate, allocated once like stream scratch
        wr = torch.zeros(rows, dtype=torch.int32, device="cuda")
        wc = torch.zeros(n, dtype=torch.int32, device="cuda")
        wb = torch.zeros(n, dtype=torch.int32, device="cuda")
        tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        L = device._lib.lib()

        def composed(i):
            device.transpose(src[i % rot], D=tr)
            device.row_weights(tr, out=wb.data_ptr())

        launches = {
            "rows": lambda i: device.row_weights(src[i % rot], out=wr.data_ptr()),
            "cols": lambda i: device.col_weights(src[i % rot], out=wc.data_ptr()),
            "b_composed": composed,
            "c_copy": lambda i: device.copy_block(dst[i % 3], 0, 0, src[i % rot], 0, 0, rows, n),
        }
        if rows == n or args.small:
            launches["total"] = lambda i: L.gf2_count_ones_dev(src[i % rot]._on(None), tot.data_ptr(), None)
        t = timed_together(launches)
        device.row_weights(src[0], out=wr.data_ptr())
        device.col_weights(src[0], out=wc.data_ptr())
        device.transpose(src[0], D=tr)
        device.row_weights(tr, out=wb.data_ptr())
        total = device.count_ones(src[0])
        same = bool((wc == wb).all()) and int(wr.sum(dtype=torch.int64)) == int(wc.sum(dtype=torch.int64)) == total
        plan = device.weights_plan("cols", rows, n)
        report("weights", [rows, n], nbytes, t, {
            "cols_over_composed": round(t["cols"][0] / t["b_composed"][0], 3), "cols_plan": list(plan), "buffers": rot,
            "row_variant": device.weights_plan("rows", rows, n)[0], "same_counts": same})
        del src, dst, tr
        torch.cuda.empty_cache()

    # select: about 0.1 % of 2^20 weights match
    n = 4096 if args.small else 1 << 20
    rng = np.random.default_rng(2026)
    rot = 3 if args.small else 96   # 4 MiB each
    ws = [torch.from_numpy(rng.integers(0, 1000, n).astype(np.int32)).cuda() for _ in range(rot)]
    copies = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = timed_together({
        "select": lambda i: device.select_weights(ws[i % rot].data_ptr(), n, 0, 0, idx=idx.data_ptr(), cap=n, count=cnt.data_ptr()),
        "c_copy": lambda i: copies[i % 3].copy_(ws[i % rot]),
    })
    device.select_weights(ws[0].data_ptr(), n, 0, 0, idx=idx.data_ptr(), cap=n, count=cnt.data_ptr())
    torch.cuda.synchronize()
    want = np.flatnonzero(ws[0].cpu().numpy() == 0)
    same = int(cnt[0]) == len(want) and np.array_equal(idx[:len(want)].cpu().numpy(), want)
    report("select", [n], 4 * n, t, {"matches": len(want), "same_indices": bool(same)})


if __name__ == "__main__":
    main()
