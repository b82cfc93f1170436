"""The exhaustive LPN solve on the device (gf2_lpn_tally_dev, gf2_wht_dev, gf2_lpn_errors_dev, gf2_min_weight_dev) next to a plain copy
of the same bytes and, at k = 16, next to the unfused route through shipped entries.

    python tools/wht_bench.py [--reps 20] [--warmup 3] [--small]

For k = 16, 20, 24, 28, 30, in one run per k:
  pass0 ..   each pass of the transform's plan alone (gf2_wht_plan; through the library's launcher of one pass);
  wht        gf2_wht_dev, all passes;
  min        gf2_min_weight_dev over the 2^k values;
  c_copy     gf2_copy_block_dev of the array's bytes, aligned: read once and written once, which is what a pass does.
  tally_N, errors_N   gf2_lpn_tally_dev / gf2_lpn_errors_dev on N = 2^20 and 2^26 rows of 256 columns (c0 = 37, label 255), with
  pool_copy_N  a copy of that operand.  The tally's rate is reported in updates (rows) per second.
At k = 16, N = 2^20 also the unfused route on a pool of 17 columns: gf2_mul_dev into 2^16 columns plus gf2_col_weights_dev, beside
gf2_lpn_errors_dev on the same pool; the two results are compared.

One process; every launch is timed on its own with HIP events after --warmup launches, the figure is the median of --reps launches, and
the variants of a k alternate launch by launch so that they see the same machine.  The arrays rotate through as many buffers as it
takes to hold 768 MiB (at least three), so that no launch finds its data in the 256 MiB last-level cache.  One JSON line per k;
profiles/wht_bench.txt keeps a run."""
import argparse
import ctypes
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
    one_pass = L.gf2k_wht_pass   # the launcher of one pass of the plan (csrc/wht/gf2_wht.h): f, k, pass, fold, n, stream -> hipError_t
    one_pass.restype = ctypes.c_int
    one_pass.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p]

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

    def as_matrix(t):
        """a contiguous tensor's bytes as a device matrix of 8 KiB rows (or one shorter row), for gf2_copy_block_dev"""
        nbytes = t.numel() * t.element_size()
        row = min(nbytes, 8192)
        return device.DMat.wrap(t.data_ptr(), nbytes // row, row * 8, row // 8, keep=t)

    def rotation(nbytes):
        return 3 if args.small else max(3, -(-(768 << 20) // nbytes))

    ks = [4, 13, 16] if args.small else [16, 20, 24, 28, 30]
    Ns = [1 << 12] if args.small else [1 << 20, 1 << 26]
    pools = {}
    for N in Ns:
        rot = rotation(N * 32)
        pools[N] = [device.DMat.random(N, 256, 20 + i) for i in range(rot)]
    pool_dst = {N: device.DMat(N, 256) for N in Ns}

    for k in ks:
        n, nbytes = 1 << k, 4 << k
        if n < 16:
            continue
        rot = rotation(nbytes)
        gen = torch.Generator(device="cuda").manual_seed(k)
        bufs = torch.randint(-(1 << 20), 1 << 20, (rot, n), dtype=torch.int32, device="cuda", generator=gen)
        dst = torch.empty((2, n), dtype=torch.int32, device="cuda")
        mats, dmats = [as_matrix(bufs[i]) for i in range(rot)], [as_matrix(dst[i]) for i in range(2)]
        out = torch.zeros(4, dtype=torch.int32, device="cuda")
        passes, bounds = device.wht_plan(k)[:2]
        launches = {}
        for p in range(passes):
            launches["pass%d" % p] = lambda i, p=p: one_pass(bufs[i % rot].data_ptr(), k, p, 0, 0, None)
        launches["wht"] = lambda i: device.wht(bufs[i % rot].data_ptr(), k)
        launches["min"] = lambda i: device.min_weight(bufs[i % rot].data_ptr(), n, idx=out.data_ptr(), val=out.data_ptr() + 4)
        launches["c_copy"] = lambda i: device.copy_block(dmats[i % 2], 0, 0, mats[i % rot], 0, 0, mats[0].nrows, mats[0].ncols)
        for N in Ns:
            r = len(pools[N])
            launches["tally_%d" % N] = lambda i, N=N, r=r: device.lpn_tally(pools[N][i % r], 37, k, 255, out=dst[i % 2].data_ptr())
            launches["errors_%d" % N] = lambda i, N=N, r=r: device.lpn_errors(pools[N][i % r], 37, k, 255, out=dst[i % 2].data_ptr())
            launches["pool_copy_%d" % N] = lambda i, N=N, r=r: device.copy_block(pool_dst[N], 0, 0, pools[N][i % r], 0, 0, N, 256)
        t = timed_together(launches)
        res = {"what": "wht", "k": k, "array_bytes": nbytes, "buffers": rot, "levels_of_each_pass": [b - a for a, b in zip(bounds, bounds[1:])],
               "tally_variant": device.wht_plan(k)[4]}
        copy = t["c_copy"][0]
        for name, (med, lo, hi) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            if name.startswith("pass"):
                res[name + "_over_copy"] = round(med / copy, 3)
                res[name + "_TBps"] = round(2 * nbytes / med / 1e9, 3)
            if name.startswith("tally_"):
                N = int(name[6:])
                res[name + "_Gupdates_per_s"] = round(N / med / 1e6, 2)
                res[name + "_over_pool_copy"] = round(med / t["pool_copy_%d" % N][0], 3)
        res["wht_over_copy"] = round(t["wht"][0] / copy, 3)
        res["sum_of_passes_ms"] = round(sum(t["pass%d" % p][0] for p in range(passes)), 4)
        for N in Ns:   # what the fold of (N - F) / 2 into the last pass saves is one more pass: errors against tally + transform
            res["errors_%d_minus_tally_and_wht_ms" % N] = round(t["errors_%d" % N][0] - t["tally_%d" % N][0] - t["wht"][0], 4)
        print(json.dumps(res), flush=True)
        del bufs, dst, mats, dmats, launches
        torch.cuda.empty_cache()
    del pools, pool_dst

    # the unfused route at k = 16: E = pool * [S ; 1] with S = all 2^16 vectors, then the column weights
    k, N = (8, 1 << 12) if args.small else (16, 1 << 20)
    n = 1 << k
    import numpy as np
    import gf2util as g
    s1 = np.ones((k + 1, n), dtype=np.uint8)
    for j in range(k):
        s1[j] = (np.arange(n) >> j) & 1
    S1 = device.DMat.from_words(g.bits_to_words(s1), n)
    rot = 3
    ps = [device.DMat.random(N, k + 1, 50 + i) for i in range(rot)]
    E = device.DMat(N, n)
    fused = torch.zeros(n, dtype=torch.int32, device="cuda")
    unfused = torch.zeros(n, dtype=torch.int32, device="cuda")

    def product_route(i):
        device.mul(ps[i % rot], S1, C=E)
        device.col_weights(E, out=unfused.data_ptr())

    t = timed_together({
        "errors": lambda i: device.lpn_errors(ps[i % rot], 0, k, k, out=fused.data_ptr()),
        "product_and_col_weights": product_route,
    })
    device.lpn_errors(ps[0], 0, k, k, out=fused.data_ptr())
    product_route(0)
    torch.cuda.synchronize()
    res = {"what": "unfused", "k": k, "N": N, "E_bytes": N * n // 8, "same_counts": bool(torch.equal(fused, unfused))}
    for name, (med, lo, hi) in t.items():
        res[name + "_ms"] = round(med, 4)
        res[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
    res["unfused_over_errors"] = round(t["product_and_col_weights"][0] / t["errors"][0], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
