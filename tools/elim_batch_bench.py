"""Batched elimination of small matrices (gf2_echelonize_batch_dev, gf2_inverse_batch_dev) next to the two yardsticks of the same run:
the loop over gf2_echelonize_dev / gf2_inverse_dev that a caller had to write before, and a plain copy_ of the stack's bytes.

    python tools/elim_batch_bench.py [--reps 9] [--warmup 2] [--loop 256] [--mib 64]

Echelon form (full = 1) of stacks of 10 x 10, 64 x 64, 128 x 128, 256 x 256 and 512 x 512 matrices and the inverse at 64 and 256.  A
stack is --mib MiB of matrices or 4096 matrices, whichever is larger; rows sit at the even stride of a gf2_dmat, and one-word rows are
timed at ld = 1 as well (what gf2_dmat_alloc gives them: dense) -- at ld = 2 half of the stack's bytes are padding that `copy_` moves
and the kernel never uses, so `stack_GBps_read_plus_written` and `rate_over_copy` count bytes of the STACK, not of the matrices.  The inputs are random:
a master copy is restored into the working stack before every run, outside the timed region, so no run finds a reduced matrix.  Every
batched call is timed on its own with HIP events after --warmup calls; the figure is the median of --reps.  `copy_` is torch's
device-to-device copy of the whole stack (it reads and writes the same bytes as the echelon form does; the inverse reads A and writes
about 29 % of Ainv).  The loop runs over the first --loop matrices of the same stack as DMat.wrap views, timed by the host clock around
the synchronous calls, median of three passes.  After the timing the batched result is compared with the loop's result on those
matrices (bit for bit, ranks and singular flags included).  `one_column_ms` is the batched call with ncols_limit = 1: the same loads,
stores and waves with the column loop cut to one column, i.e. what the memory access pattern alone costs.
One JSON line per measurement; profiles/elim_batch_bench.txt keeps a run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (call, n, row stride in words; None: the width rounded up to even, a gf2_dmat's rule).  One-word rows are timed in both layouts a caller
# meets: ld = 1 is what gf2_dmat_alloc gives them (dense: every byte of the stack is a matrix word), ld = 2 carries a padding word per row
CASES = [("echelon", 10, 1), ("echelon", 10, 2), ("echelon", 64, 1), ("echelon", 64, 2), ("echelon", 128, None), ("echelon", 256, None),
         ("echelon", 512, None), ("inverse", 64, 1), ("inverse", 64, 2), ("inverse", 256, None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop", type=int, default=256)
    ap.add_argument("--mib", type=int, default=64)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from m4ri_rust_amd import _lib, device
    device.require_gpu()
    L = _lib.lib()

    def event_ms(launch):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def median_ms(launch, prepare):
        ts = []
        for i in range(args.warmup + args.reps):
            prepare()
            t = event_ms(launch)
            if i >= args.warmup:
                ts.append(t)
        return statistics.median(ts), min(ts), max(ts)

    for what, n, ld in CASES:
        if ld is None:
            ld = ((n + 63) // 64 + 1) & ~1
        per_matrix = n * ld * 8
        batch = max(4096, (args.mib << 20) // per_matrix)
        rows = batch * n
        master = torch.empty((rows, ld), dtype=torch.int64, device="cuda")
        device.DMat.from_torch(master, n).fill_random(1000 + n)
        if ld > (n + 63) // 64:
            master[:, (n + 63) // 64:] = 0  # the padding word of the even stride
        work, out = torch.empty_like(master), torch.zeros_like(master)
        ranks = torch.zeros(batch, dtype=torch.int32, device="cuda")
        flags = torch.zeros(batch, dtype=torch.int32, device="cuda")
        W, O = device.DMat.from_torch(work, n), device.DMat.from_torch(out, n)
        plan = device.elim_batch_plan(n, n, inverse=what == "inverse")

        if what == "echelon":
            def batched():
                device.echelonize_batch(W, n, full=True, ranks=ranks.data_ptr(), pivots=device.SKIP)
        else:
            def batched():
                device.inverse_batch(W, n, Ainv=O, singular=flags.data_ptr())
        t_batch = median_ms(batched, lambda: work.copy_(master))
        # the same kernel with the column loop cut to ONE column: what loading, storing and starting the waves cost without the elimination
        t_io = None
        if what == "echelon":
            t_io = median_ms(lambda: device.echelonize_batch(W, n, full=True, ncols_limit=1, ranks=ranks.data_ptr(), pivots=device.SKIP),
                             lambda: work.copy_(master))
        t_copy = median_ms(lambda: work.copy_(master), lambda: None)

        # the loop a caller had to write: one synchronous call per matrix
        k = min(args.loop, batch)
        loop_in, loop_out = torch.empty((k * n, ld), dtype=torch.int64, device="cuda"), torch.zeros((k * n, ld), dtype=torch.int64, device="cuda")
        views = [device.DMat.wrap(loop_in.data_ptr() + 8 * b * n * ld, n, n, ld) for b in range(k)]
        oviews = [device.DMat.wrap(loop_out.data_ptr() + 8 * b * n * ld, n, n, ld) for b in range(k)]
        loop_ranks, loop_flags = [0] * k, [0] * k
        r = ctypes.c_int(0)
        passes = []
        for _ in range(4):
            loop_in.copy_(master[:k * n])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(k):
                if what == "echelon":
                    _lib.check(L.gf2_echelonize_dev(ctypes.byref(views[b].s), 1, 0, ctypes.byref(r), None, None), "gf2_echelonize_dev")
                    loop_ranks[b] = r.value
                else:
                    _lib.check(L.gf2_inverse_dev(ctypes.byref(oviews[b].s), ctypes.byref(views[b].s), ctypes.byref(r), None), "gf2_inverse_dev")
                    loop_flags[b] = r.value
            torch.cuda.synchronize()
            passes.append((time.perf_counter() - t0) * 1e3)
        t_loop = statistics.median(passes[1:])

        # same bits as the loop
        work.copy_(master)
        batched()
        torch.cuda.synchronize()
        if what == "echelon":
            same = bool(torch.equal(work[:k * n], loop_in)) and ranks[:k].cpu().tolist() == loop_ranks
        else:
            fl = flags[:k].cpu().tolist()
            same = fl == loop_flags and all(fl[b] or bool(torch.equal(out[b * n:(b + 1) * n], loop_out[b * n:(b + 1) * n])) for b in range(k))
        med, lo, hi = t_batch
        stack_bytes = rows * ld * 8
        print(json.dumps({
            "what": what, "n": n, "ld": ld, "batch": batch, "stack_MiB": round(stack_bytes / 2**20, 1), "variant": plan[0], "threads": plan[1],
            "matrices_per_workgroup": plan[2], "lds_bytes": plan[3],
            "batched_ms": round(med, 4), "batched_ms_min": round(lo, 4), "batched_ms_max": round(hi, 4),
            "matrices_per_s": round(batch / med * 1e3), "us_per_matrix": round(med * 1e3 / batch, 4),
            "stack_GBps_read_plus_written": round(2 * stack_bytes / med / 1e6, 1),
            "one_column_ms": round(t_io[0], 4) if t_io else None,
            "copy_ms": round(t_copy[0], 4), "copy_GBps": round(2 * stack_bytes / t_copy[0] / 1e6, 1),
            "rate_over_copy": round(t_copy[0] / med, 4),
            "loop_matrices": k, "loop_us_per_matrix": round(t_loop * 1e3 / k, 2), "loop_matrices_per_s": round(k / t_loop * 1e3),
            "loop_over_batched_per_matrix": round((t_loop / k) / (med / batch), 1), "same_bits_as_loop": same}), flush=True)
        del master, work, out, loop_in, loop_out, views, oviews, W, O
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
