"""Device-resident null space (gf2_nullspace_dev) next to the elimination alone, the assembly launch alone, a plain copy of the
assembly's byte count, and the route a caller had to take before: echelonize, download, gather the free columns on the host, upload.

    python tools/nullspace_bench.py [--shapes random:4096x8192,random:32768x65536,alternating:16384] [--reps 3] [--no-host-route]

Shapes: `random:MxN` is a seeded random matrix (full row rank; its pivots come first but for the few columns a random matrix skips);
`alternating:N` is N x N of rank N / 2 whose pivot columns are the odd ones -- every source word goes through the bit compress.
All device times are HIP events on the stream of the calls, in ms, the median of --reps runs after one warm-up run; the three device
figures of a shape come from one process.  The assembly's bytes are what the algorithm needs: each pivot row reads every source word
that holds a free column once, and every word of K is written once.  One JSON line per shape; profiles/nullspace_bench.txt keeps a
run."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def alternating_factor(n):
    """E (n / 2 x n words): row i has its pivot at column 2 i + 1, random bits at the even columns right of it, zeros elsewhere"""
    rng = np.random.default_rng(7)
    r, w = n // 2, n // 64
    e = rng.integers(0, 1 << 63, size=(r, w), dtype=np.uint64) & np.uint64(0x5555555555555555)
    piv = 2 * np.arange(r) + 1
    q = np.arange(w)[None, :]
    pw, pb = (piv >> 6)[:, None], (piv & 63)[:, None].astype(np.uint64)
    above = ~((np.uint64(2) << pb) - np.uint64(1))  # bits right of the pivot
    e = np.where(q < pw, np.uint64(0), np.where(q == pw, (e & above) | (np.uint64(1) << pb), e))
    return np.ascontiguousarray(e)


def host_gather(e_words, piv, n):
    """what a caller did on the host: K from the downloaded reduced form (numpy on unpacked bits)"""
    r = len(piv)
    free = np.setdiff1d(np.arange(n), np.asarray(piv, dtype=np.int64))
    bits = np.unpackbits(e_words[:r].view(np.uint8).reshape(r, -1), axis=1, bitorder="little")[:, :n]
    k = np.zeros((n, len(free)), dtype=np.uint8)
    k[free, np.arange(len(free))] = 1
    k[np.asarray(piv, dtype=np.int64)] = bits[:, free]
    pad = (-len(free)) % 64
    if pad:
        k = np.hstack([k, np.zeros((n, pad), dtype=np.uint8)])
    return np.packbits(k, axis=1, bitorder="little").view(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="random:4096x8192,random:32768x65536,alternating:16384")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host-route", action="store_true", help="skip echelonize + download + host gather + upload")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from m4ri_rust_amd import _lib, device
    device.require_gpu()
    L = _lib.lib()

    def events(fn):
        """median event time of fn() over the repetitions; fn prepares (untimed) and returns the call to time"""
        ts = []
        for _ in range(args.reps + 1):
            call = fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts[1:])

    for spec in args.shapes.split(","):
        kind, dims = spec.split(":")
        if kind == "random":
            m, n = (int(x) for x in dims.split("x"))
            src = device.DMat.random(m, n, 1)
        else:
            m = n = int(dims)
            src = device.mul(device.DMat.random(n, n // 2, 1), device.DMat.from_words(alternating_factor(n), n))
        out = {"shape": spec, "m": m, "n": n}
        res = {}

        def nullspace_call():
            A = src.clone()
            res.clear()

            def call():
                res["K"], res["rank"], res["piv"] = device.nullspace(A)
            return call

        def echelonize_call():
            A = src.clone()
            return lambda: device.echelonize(A, full=True)

        asm = []

        def assembly_only():  # the library's own events around the assembly launch
            device.prof_enable(True)
            device.nullspace(src.clone())
            device.prof_enable(False)
            device.prof_read(reset=True)  # the product launches of the elimination were timed too: drop them
            asm.append(L.gf2_nullspace_last_assembly_ms())
        for _ in range(args.reps + 1):
            assembly_only()
        out["nullspace_ms"] = round(events(nullspace_call), 3)
        out["echelonize_ms"] = round(events(echelonize_call), 3)
        out["assembly_ms"] = round(statistics.median(asm[1:]), 4)
        rank, piv = res["rank"], np.asarray(res["piv"], dtype=np.int64)
        d = n - rank
        kw = (d + 63) // 64
        free_words = len(np.unique(np.setdiff1d(np.arange(n), piv) >> 6))
        rd, wr = rank * free_words * 8, n * kw * 8
        out.update(rank=rank, pivots_beyond_rank=int((piv >= rank).sum()),  # 0: the pivots are exactly the first `rank` columns
                   assembly_read_bytes=rd, assembly_write_bytes=wr,
                   assembly_GBps=round((rd + wr) / out["assembly_ms"] / 1e6, 1))
        # a plain device-to-device copy that moves the same bytes (half read, half written)
        half = (rd + wr) // 2 // 8
        a_buf = torch.empty(half, dtype=torch.int64, device="cuda")
        b_buf = torch.ones(half, dtype=torch.int64, device="cuda")
        out["copy_ms"] = round(events(lambda: (lambda: a_buf.copy_(b_buf))), 4)
        out["copy_GBps"] = round(2 * half * 8 / out["copy_ms"] / 1e6, 1)
        out["assembly_over_copy_rate"] = round(out["assembly_GBps"] / out["copy_GBps"], 3)
        del a_buf, b_buf
        k_dev = res["K"].to_words() if not args.no_host_route and n <= 16384 else None
        res.clear()
        if not args.no_host_route:
            # the route without gf2_nullspace_dev, wall clock (it ends on the host): every step is public API of the parent commit
            ts = []
            for _ in range(2 if m * n <= 1 << 28 else 1):  # the host gather of 32768 x 65536 works on gigabytes of unpacked bits
                A = src.clone()
                device.equal(A, A)  # drain the queue
                t0 = time.perf_counter()
                r2, piv2 = device.echelonize(A, full=True)
                t1 = time.perf_counter()
                e = A.to_words()
                t2 = time.perf_counter()
                k = host_gather(e, piv2, n)
                t3 = time.perf_counter()
                K2 = device.DMat.from_words(k, n - r2)
                device.equal(K2, K2)
                t4 = time.perf_counter()
                ts.append([(y - x) * 1e3 for x, y in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t0, t4))])
            best = min(ts, key=lambda t: t[4])
            for name, v in zip(("echelonize", "download", "host_gather", "upload", "total"), best):
                out["host_route_%s_ms" % name] = round(v, 2)
            out["host_route_over_nullspace"] = round(best[4] / out["nullspace_ms"], 1)
            if k_dev is not None:
                out["host_route_same_bits"] = bool(np.array_equal(k, k_dev))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
