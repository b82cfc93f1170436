"""The Hamming-distance search (gf2_near_pairs_dev, gf2_nearest_dev) next to the join with an empty window (gf2_join_select_dev, b == 0),
which was the only route to "pairs within a radius" before it, and next to a plain copy of the two pools.

    python tools/near_bench.py [--reps 5] [--warmup 1] [--small] [--max-seconds 4]

The pools of profiles/join_select_bench.txt: 256 columns of random bits, distances over the columns [70, 256), 186 columns, device
resident; NA = NB = 2^16 and 2^18, and 2^20 (one run per variant) if the runs at 2^18 say that one stays under --max-seconds.
Per shape:
  near_none       gf2_near_pairs_dev with the window [0, 20]: no pair is that near;
  near_1e-4       ... with [0, q], q the 1e-4 quantile of the binomial distribution of 186 fair bits: about one hit per 10^4 pairs,
                  with D, ia, ib and wt at a capacity of 1.2 times the hits expected; the observed rate is printed;
  nearest         gf2_nearest_dev with idx and dist;
  join_none / join_1e-4   gf2_join_select_dev with b == 0 and the same windows and outputs: the same bits (compared before the timing);
  copy            a plain copy of A and of B (hipMemcpyAsync through torch): what reading both pools once costs.
Pairs per second are NA * NB over the time; `of_ceiling` is that rate over the vector issue limit of the kernel that ran: the vector
instructions per pair and lane of the inner loop of gf2_near_kernel<4, .> as counted in the shipped ISA (VALU_PER_PAIR below: 16 for the
XORs and popcounts of eight 32-bit words, the rest sums the words and applies the window or the minimum), at 256 CUs x 4 SIMDs x 32
lanes per clock and the peak engine clock of 2.4 GHz (--clock-mhz overrides it; the clock held under load is lower and is not read
here, so the ceiling is an upper one and `of_ceiling` a lower bound of the share of the issue slots in use).

One process; every variant is timed on its own with HIP events after --warmup runs, the figure is the median of --reps runs, and the
variants of a shape alternate run by run so that they see the same machine.  One JSON line per shape; profiles/near_bench.txt keeps
a run."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS, WC0, WC1 = 256, 70, 256
WIDTH = WC1 - WC0
VALU_PER_PAIR = {"pairs": 169 / 8, "nearest": 157 / 8}       # gf2_near_kernel<4, kNearCount / kNearNearest>: per eight pairs of the unrolled loop
LANES_PER_CLOCK = 256 * 4 * 32
PEAK_MHZ = 2400.0            # the engine clock of the MI355X at its peak; under load the chip holds less, so the ceiling is an upper one


def binomial_quantile(n, p):
    """(the largest q with P(X <= q) <= p for X the number of ones of n fair bits, that probability)"""
    total, acc, q = 2 ** n, 0, -1
    while (acc + math.comb(n, q + 1)) <= p * total:
        q += 1
        acc += math.comb(n, q)
    return q, acc / total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes (overheads, not rates)")
    ap.add_argument("--max-seconds", type=float, default=4.0, help="the largest shape runs only if one run is expected to stay below this")
    ap.add_argument("--clock-mhz", type=float, default=0.0, help="the engine clock of the ceiling (default: the peak, 2400)")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from m4ri_rust_amd import device
    device.require_gpu()
    L = device._lib.lib()
    mhz = args.clock_mhz or PEAK_MHZ
    ceiling = {k: LANES_PER_CLOCK * mhz * 1e6 / v for k, v in VALU_PER_PAIR.items()}

    def timed_together(launches, reps, warmup):
        ts = {k: [] for k in launches}
        for i in range(warmup + reps):
            for name, launch in launches.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    ts[name].append(a.elapsed_time(b))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    ints = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")  # noqa: E731
    ld = NCOLS // 64
    q4, p4 = binomial_quantile(WIDTH, 1e-4)
    windows = [("none", 20, 0.0), ("1e-4", q4, p4)]
    two = torch.zeros(4, dtype=torch.int64, device="cuda")
    cp, hp = two.data_ptr(), two.data_ptr() + 8
    for log_n in (8, 10) if args.small else (16, 18, 20):
        N = 1 << log_n
        pairs = N * N
        largest = log_n == 20
        ta, tb, ca, cb = (torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(4))
        A, B = device.DMat.from_torch(ta, NCOLS), device.DMat.from_torch(tb, NCOLS)
        A.fill_random(40 + log_n)
        B.fill_random(140 + log_n)
        idx, dist = ints(N), ints(N)
        plan = device.near_plan(N, N, NCOLS, (WC0, WC1))
        res = {"what": "near", "NA": N, "NB": N, "pairs": pairs, "kernel_words": plan[0], "chunks": plan[3], "rows_per_chunk": plan[4],
               "scratch_bytes": plan[6], "clock_mhz": mhz, "valu_per_pair": {k: round(v, 2) for k, v in VALU_PER_PAIR.items()},
               "ceiling_pairs_per_s": {k: float("%.4g" % v) for k, v in ceiling.items()}}
        launches, outs = {}, {}
        for name, whi, prob in windows:
            hcap = max(int(1.2 * prob * pairs), 1024)
            outs[name] = [device.DMat(hcap, NCOLS), device.DMat(hcap, NCOLS)] + [ints(hcap) for _ in range(6)]
            Dn, Dj, na_, nb_, nw_, ja_, jb_, jw_ = outs[name]
            launches["near_" + name] = (lambda whi=whi, Dn=Dn, a=na_, b=nb_, w=nw_: device.near_pairs(
                A, B, (WC0, WC1), 0, whi, D=Dn, hits=hp, ia=a.data_ptr(), ib=b.data_ptr(), wt=w.data_ptr()))
            launches["join_" + name] = (lambda whi=whi, Dj=Dj, a=ja_, b=jb_, w=jw_: device.join_select(
                A, B, 0, 0, (WC0, WC1), 0, whi, D=Dj, count=cp, hits=hp, ia=a.data_ptr(), ib=b.data_ptr(), wt=w.data_ptr()))
        launches["nearest"] = lambda: device.nearest(A, B, (WC0, WC1), idx=idx.data_ptr(), dist=dist.data_ptr())
        launches["copy"] = lambda: (ca.copy_(ta), cb.copy_(tb))
        # the largest shape: one run of each variant, and only what is expected to stay under --max-seconds (16 times the time at 2^18)
        if largest:
            expected = {k: 16 * v / 1000.0 for k, v in last_ms.items()}
            skipped = sorted(k for k, v in expected.items() if v > args.max_seconds)
            launches = {k: v for k, v in launches.items() if k not in skipped}
            res["not_run"] = {k: "expected %.1f s per run" % expected[k] for k in skipped}
        # the two routes agree before they are timed
        for name, whi, prob in windows:
            if "near_" + name not in launches:
                continue
            launches["near_" + name]()
            torch.cuda.synchronize()
            hits = int(two[1])
            res["hits_" + name] = hits
            res["observed_rate_" + name] = hits / pairs
            Dn, Dj, na_, nb_, nw_, ja_, jb_, jw_ = outs[name]
            if "join_" + name in launches:
                launches["join_" + name]()
                torch.cuda.synchronize()
                n = min(hits, Dn.nrows)
                assert int(two[1]) == hits and int(two[0]) == pairs, (int(two[1]), hits)
                assert all(torch.equal(x[:n], y[:n]) for x, y in ((na_, ja_), (nb_, jb_), (nw_, jw_)))
                k = min(n, 1 << 16)
                if k:
                    assert (device.submatrix(Dn, 0, 0, k, NCOLS).to_words() == device.submatrix(Dj, 0, 0, k, NCOLS).to_words()).all()
        t = timed_together(launches, 1 if largest else args.reps, 0 if largest else args.warmup)
        last_ms = {k: v[0] for k, v in t.items()}
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
            if name != "copy":
                rate = pairs / (med / 1000.0)
                res[name + "_pairs_per_s"] = float("%.4g" % rate)
                if not name.startswith("join_"):
                    res[name + "_of_ceiling"] = round(rate / ceiling["nearest" if name == "nearest" else "pairs"], 3)
        for name, _, _ in windows:
            if "join_" + name in t and "near_" + name in t:
                res["near_over_join_" + name] = round(t["near_" + name][0] / t["join_" + name][0], 4)
        print(json.dumps(res), flush=True)
        del A, B, ta, tb, ca, cb, outs, launches, idx, dist
        torch.cuda.empty_cache()
        L.gf2_trim()


if __name__ == "__main__":
    main()
