"""One LF2 round of a BKW reduction on the device (gf2_lf2_reduce_dev) and the stable class sort under it (gf2_class_sort_dev), next
to a plain copy of the pool's bytes, an LF1 round of the same pool, the route without the fused pair kernel, and a library radix sort.

    python tools/lf2_bench.py [--reps 20] [--warmup 3] [--small] [--build-only]

Pools of 256 columns of random bits, window c0 = 37, N = 3 * 2^b rows for b = 18, 22, 24, capacity 1.6 N; for every b, in one run:
  reduce        gf2_lf2_reduce_dev: the sort, pair count, scan, pair scatter;
  sort          gf2_class_sort_dev alone; pass_0, pass_1, ... its passes singly through the library's launcher (csrc/lf2/gf2_lf2.h:
                count, three scan launches, scatter), each on the pairs the pass before it left for pool 0 (pass_0 reads the rotating
                pools; the later ones read one pair buffer of 8 N bytes, which at b = 18 fits the last-level cache);
  pair_count, pair_scatter   the launches of the pairs singly, on the sorted order of the same pool made beforehand;
  two_gathers   gf2_gather_rows_dev(D, P, hi) then gf2_gather_rows_dev(D, P, lo, accumulate) on finished lo / hi arrays: the composed
                route, which would still need a launch that writes lo and hi (8 bytes per output) on top;
  pool_copy     gf2_copy_block_dev of the pool's bytes;
  lf1_reduce    one gf2_lf1_reduce_dev round of the same pool and b;
  rocprim_sort  rocprim::radix_sort_pairs of the same (key, row) pairs, b key bits, from the headers of the ROCm tree, where they are
                there: built by this tool into tools/lf2_rocprim_sort.so, never part of the library or of a test.  Its keys are
                extracted beforehand, so it reads 4 bytes per row where pass_0 reads a row's key word out of the pool.
At b = 18 also the host route that the entry replaces, once: download, the numpy yardstick of tests/lf2_ref.py, upload.

One process; every launch is timed on its own with HIP events after --warmup launches, the figure is the median of --reps launches, and
the variants of a shape alternate launch by launch so that they see the same machine.  The pools rotate through as many buffers as it
takes to hold 768 MiB (at least three).  One JSON line per shape; profiles/lf2_bench.txt keeps a run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS, C0 = 256, 37
ROCPRIM_SO = os.path.join(ROOT, "tools", "lf2_rocprim_sort.so")
ROCPRIM_SRC = r"""
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
extern "C" int lf2_rocprim_sort(void *tmp, size_t *tmp_bytes, const unsigned *keys_in, unsigned *keys_out, const int *rows_in,
                                int *rows_out, size_t n, int bits, hipStream_t stream) {
  return (int)rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys_in, keys_out, rows_in, rows_out, n, 0u, (unsigned)bits, stream);
}
"""


def rocprim_sort():
    """the comparison sort as a ctypes function, or None with the reason"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.exists(os.path.join(rocm, "include", "rocprim", "device", "device_radix_sort.hpp")):
        return None, "no rocPRIM headers under %s" % rocm
    if not os.path.exists(ROCPRIM_SO):
        with tempfile.TemporaryDirectory() as tmp:
            src = os.path.join(tmp, "lf2_rocprim_sort.hip")
            with open(src, "w") as f:
                f.write(ROCPRIM_SRC)
            try:
                subprocess.check_call([os.path.join(rocm, "bin", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src,
                                       "-o", ROCPRIM_SO])
            except (OSError, subprocess.CalledProcessError) as e:
                return None, "the rocPRIM sort did not build: %s" % e
    fn = ctypes.CDLL(ROCPRIM_SO).lf2_rocprim_sort
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)] + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return fn, "rocprim::radix_sort_pairs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not rates)")
    ap.add_argument("--build-only", action="store_true", help="build the library and the comparison sort, then stop")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    rp_sort, rp_note = rocprim_sort()
    if args.build_only:
        print(rp_note)
        return
    import numpy as np
    import torch
    from m4ri_rust_amd import device
    device.require_gpu()
    L = device._lib.lib()
    I, P, LL = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    k_pass, k_count, k_scatter = L.gf2k_lf2_sort_pass, L.gf2k_lf2_pair_count, L.gf2k_lf2_pair_scatter
    for fn, argtypes in ((k_pass, [P, LL, I, I, P, I, I, P, P, P, P, P, P]), (k_count, [P, I, P, P, P]),
                         (k_scatter, [P, LL, I, I, P, P, P, P, LL, I, P, P, I, P])):
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
                launch(i)
                b.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ts[name].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    print(json.dumps({"what": "comparison sort", "note": rp_note}), flush=True)
    ints = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")  # noqa: E731
    ld = NCOLS // 64
    bs = [8] if args.small else [18, 22, 24]
    for b in bs:
        N = 3 << b
        cap = int(1.6 * N)
        rot = 3 if args.small else max(3, -(-(768 << 20) // (N * 32)))
        tensors = [torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(rot)]
        pools = [device.DMat.from_torch(t, NCOLS) for t in tensors]
        for i, p in enumerate(pools):
            p.fill_random(40 + i)
        plan = device.lf2_plan(N, NCOLS, b)
        passes, T, R, lanes = plan[0], plan[4], plan[5], plan[6]
        tiles, runs = -(-N // T), -(-N // R)
        dst = device.DMat(cap, NCOLS)
        dstN = device.DMat.wrap(dst.s.data, N, NCOLS, dst.ld, keep=dst)
        lo, hi, order, skeys, src = ints(cap), ints(cap), ints(N), ints(N), ints(N)
        count = torch.zeros(2, dtype=torch.int64, device="cuda")
        pairs = [torch.zeros((N, 2), dtype=torch.int32, device="cuda") for _ in range(2)]
        counts, parts = ints(256 * tiles), ints(256 * tiles // 2048 + 1)
        first = ints(1 << b)
        # per pool, beforehand: the sorted order, the run offsets, lo and hi
        state = []
        for p in pools:
            o, k, s = ints(N), ints(N), torch.zeros(runs, dtype=torch.int64, device="cuda")
            device.class_sort(p, C0, b, order=o.data_ptr(), skeys=k.data_ptr())
            ok(k_count(k.data_ptr(), N, s.data_ptr(), count.data_ptr(), None))
            l, h = ints(cap), ints(cap)
            device.lf2_reduce(p, C0, b, D=dst, count=count.data_ptr(), lo=l.data_ptr(), hi=h.data_ptr())
            torch.cuda.synchronize()
            state.append((o, k, s, l, h, int(count[0])))
        pool = lambda i: pools[i % rot]  # noqa: E731
        cp, lp, hp = count.data_ptr(), lo.data_ptr(), hi.data_ptr()

        def sort_pass(i, j, P0=None):
            first_pass, last = j == 0, j == passes - 1
            ok(k_pass((P0 if P0 is not None else pools[0]).s.data if first_pass else None, ld, C0, b, None if first_pass else pairs[(j - 1) & 1].data_ptr(), N, j,
                      counts.data_ptr(), parts.data_ptr(), None if last else pairs[j & 1].data_ptr(), order.data_ptr() if last else None,
                      skeys.data_ptr() if last else None, None))

        for j in range(passes):          # the state every later pass is timed on
            sort_pass(0, j)
        torch.cuda.synchronize()

        def pair_scatter(i):
            o, k, s, _, _, _ = state[i % rot]
            ok(k_scatter(pool(i).s.data, ld, N, NCOLS, o.data_ptr(), k.data_ptr(), s.data_ptr(), dst.s.data, dst.ld, cap, lp, hp, -1, None))

        def two_gathers(i):
            _, _, _, l, h, n = state[i % rot]
            view = device.DMat.wrap(dst.s.data, min(n, cap), NCOLS, dst.ld, keep=dst)
            device.gather_rows(pool(i), h.data_ptr(), D=view)
            device.gather_rows(pool(i), l.data_ptr(), D=view, accumulate=True)

        launches = {
            "reduce": lambda i: device.lf2_reduce(pool(i), C0, b, D=dst, count=cp, lo=lp, hi=hp),
            "sort": lambda i: device.class_sort(pool(i), C0, b, order=order.data_ptr(), skeys=skeys.data_ptr()),
            "pair_count": lambda i: ok(k_count(state[i % rot][1].data_ptr(), N, state[i % rot][2].data_ptr(), cp, None)),
            "pair_scatter": pair_scatter,
            "two_gathers": two_gathers,
            "pool_copy": lambda i: device.copy_block(dstN, 0, 0, pool(i), 0, 0, N, NCOLS),
            "lf1_reduce": lambda i: device.lf1_reduce(pool(i), C0, b, D=dstN, first=first.data_ptr(), count=cp, src=src.data_ptr()),
        }
        launches["pass_0"] = lambda i: sort_pass(i, 0, pool(i))
        for j in range(1, passes):
            launches["pass_%d" % j] = lambda i, j=j: sort_pass(i, j)
        if rp_sort:
            keys_in = [((t[:, 0] >> C0) & ((1 << b) - 1)).to(torch.int32) for t in tensors]
            rows_in = torch.arange(N, dtype=torch.int32, device="cuda")
            need = ctypes.c_size_t(0)
            ok(rp_sort(None, ctypes.byref(need), keys_in[0].data_ptr(), skeys.data_ptr(), rows_in.data_ptr(), order.data_ptr(), N, b, None))
            tmp = torch.zeros(need.value + 16, dtype=torch.uint8, device="cuda")
            launches["rocprim_sort"] = lambda i: ok(rp_sort(tmp.data_ptr(), ctypes.byref(need), keys_in[i % rot].data_ptr(), skeys.data_ptr(),
                                                            rows_in.data_ptr(), order.data_ptr(), N, b, None))
        t = timed_together(launches)
        torch.cuda.synchronize()
        n_out = state[0][5]
        res = {"what": "lf2", "N": N, "b": b, "pool_bytes": N * 32, "buffers": rot, "capacity": cap, "pairs": n_out, "passes": passes,
               "tile_rows": T, "run_rows": R, "lanes_per_row": lanes, "sort_scratch_bytes": plan[7], "reduce_scratch_bytes": plan[8]}
        if rp_sort:     # the last launch of a shape was the comparison sort: it must have given the order of the library's
            torch.cuda.synchronize()
            got = order.clone()
            device.class_sort(pools[(args.warmup + args.reps - 1) % rot], C0, b, order=order.data_ptr(), skeys=skeys.data_ptr())
            torch.cuda.synchronize()
            res["rocprim_same_order"] = bool(torch.equal(got, order))
            res["rocprim_temp_bytes"] = int(need.value)
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
        res["sum_of_passes_ms"] = round(sum(t["pass_%d" % j][0] for j in range(passes)), 4)
        res["reduce_over_pool_copy"] = round(t["reduce"][0] / t["pool_copy"][0], 3)
        res["reduce_over_lf1_reduce"] = round(t["reduce"][0] / t["lf1_reduce"][0], 3)
        res["pair_scatter_over_two_gathers"] = round(t["pair_scatter"][0] / t["two_gathers"][0], 3)
        # the floor: passes x 16 bytes per row of the sort, two rows read and one written per output
        floor_bytes = passes * 16 * N + 3 * 32 * min(n_out, cap)
        res["floor_bytes"] = floor_bytes
        res["floor_over_pool_bytes"] = round(floor_bytes / (N * 32), 3)
        res["reduce_GBps_of_floor_bytes"] = round(floor_bytes / t["reduce"][0] / 1e6, 1)
        res["pool_copy_GBps"] = round(2 * N * 32 / t["pool_copy"][0] / 1e6, 1)
        if rp_sort:
            res["sort_over_rocprim_sort"] = round(t["sort"][0] / t["rocprim_sort"][0], 3)
        print(json.dumps(res), flush=True)
        if b == bs[0]:
            import lf2_ref as lf
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            words = pools[0].to_words()
            t1 = time.perf_counter()
            r = lf.lf2(words, NCOLS, C0, b)
            t2 = time.perf_counter()
            up = device.DMat.from_words(r.D, NCOLS)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            got = device.lf2_reduce(pools[0], C0, b)[0]
            same = bool(np.array_equal(got.to_words(), r.D))
            print(json.dumps({"what": "host route", "N": N, "b": b, "download_ms": round(1e3 * (t1 - t0), 2), "numpy_ms": round(1e3 * (t2 - t1), 2),
                              "upload_ms": round(1e3 * (t3 - t2), 2), "total_ms": round(1e3 * (t3 - t0), 2), "same_bits_as_the_device": same}),
                  flush=True)
            del up, got, words, r
        del tensors, pools, dst, dstN, lo, hi, order, skeys, src, pairs, counts, parts, first, state, launches
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
