"""The weight-filtered join (gf2_join_select_dev) next to the composed route that it replaces and to gf2_join_dev alone.

    python tools/join_select_bench.py [--reps 10] [--warmup 2] [--small]

The shapes of profiles/join_bench.txt: pools of 256 columns of random bits, window c0 = 37, NA = NB = m * 2^b rows for (b, m) = (24, 1),
(24, 4) and (18, 1); the expected count is m^2 2^b pairs; weights over the columns [70, 256), 186 columns.  Three windows of weights:
  none      [0, 20]: no pair is that light -- the Stern case, where a hit is the end of the search;
  percent   [0, q], q the 1 % quantile of the binomial distribution of 186 fair bits; the observed rate is printed;
  all       [0, 186]: every pair is a hit, the worst case: every pair is weighed twice and every row is written.
For every shape and window, in one run:
  join            gf2_join_dev alone at a capacity of 1.2 times the expected count, with ia, ib and wt: every pair is written;
  composed        the route without this entry: gf2_join_dev as above, gf2_select_weights_dev on its weights, gf2_gather_rows_dev of
                  the hits of D, and the selections of ia, ib and wt by the same indices (torch.index_select: the library has no
                  gather of ints);
  select          gf2_join_select_dev with D, ia, ib and wt at a capacity in HITS (1.2 times those expected, 1024 at the least);
  select_index    the same without rows (D->data NULL): ia, ib and wt alone;
  select_counts   the counts-only call (D->nrows == 0): the sorts, the count and the weigh pass.
A last shape that the composed route cannot run at all: b = 12, NA = NB = 2^22, 2^32 pairs (more than an int capacity holds, 176 GiB
of rows, indices and weights), with the window [0, q] of the 1e-7 quantile: join_count (the count-only gf2_join_dev), select,
select_index and select_counts.

One process; every variant is timed on its own with HIP events after --warmup runs, the figure is the median of --reps runs, and the
variants of a shape alternate run by run so that they see the same machine.  The pools do not rotate: at b = 18 the operands fit the
last-level cache.  One JSON line per shape and window; profiles/join_select_bench.txt keeps a run."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NCOLS, C0, WC0, WC1 = 256, 37, 70, 256
WIDTH = WC1 - WC0


def binomial_quantile(n, p):
    """(the largest q with P(X <= q) <= p for X the number of ones of n fair bits, that probability)"""
    total, acc, q = 2 ** n, 0, -1
    while (acc + math.comb(n, q + 1)) <= p * total:
        q += 1
        acc += math.comb(n, q)
    return q, acc / total


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

    def timed_together(launches, reps):
        ts = {k: [] for k in launches}
        for i in range(args.warmup + reps):
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
    q1, p1 = binomial_quantile(WIDTH, 0.01)
    q7, p7 = binomial_quantile(WIDTH, 1e-7)
    windows = [("none", 20, 0.0), ("percent", q1, p1), ("all", WIDTH, 1.0)]
    shapes = [(8, 1), (8, 4)] if args.small else [(24, 1), (24, 4), (18, 1)]
    big = (6, 1 << 12) if args.small else (12, 1 << 10)      # (b, m): m^2 2^b pairs

    def pools(b, m):
        N = m << b
        ta, tb = (torch.empty((N, ld), dtype=torch.int64, device="cuda") for _ in range(2))
        A, B = device.DMat.from_torch(ta, NCOLS), device.DMat.from_torch(tb, NCOLS)
        A.fill_random(40 + b)
        B.fill_random(140 + b)
        return N, A, B

    def report(res, t):
        for name, (med, lo_, hi_) in t.items():
            res[name + "_ms"] = round(med, 4)
            res[name + "_ms_min_max"] = [round(lo_, 4), round(hi_, 4)]
        print(json.dumps(res), flush=True)

    two = torch.zeros(4, dtype=torch.int64, device="cuda")
    cp, hp = two.data_ptr(), two.data_ptr() + 8
    none = device.DMat.wrap(None, 0, NCOLS, ld)
    for b, m in shapes:
        N, A, B = pools(b, m)
        expected = m * m << b
        cap = int(1.2 * expected)
        plan = device.join_select_plan(N, N, NCOLS, b, (WC0, WC1))
        D = device.DMat(cap, NCOLS)
        ia, ib, wt = ints(cap), ints(cap), ints(cap)
        device.join(A, B, C0, b, D=D, count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(), wt=wt.data_ptr(), wcols=(WC0, WC1))
        torch.cuda.synchronize()
        pairs = int(two[0])
        assert pairs <= cap
        for name, whi, prob in windows:
            hcap = max(int(1.2 * prob * expected), 1024)
            Dh, Ds = device.DMat(hcap, NCOLS), device.DMat(hcap, NCOLS)
            idx, cnt = ints(hcap), ints(1)
            sa, sb, sw = ints(hcap), ints(hcap), ints(hcap)
            unstored = device.DMat.wrap(None, hcap, NCOLS, ld)

            def composed():
                device.join(A, B, C0, b, D=D, count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(), wt=wt.data_ptr(), wcols=(WC0, WC1))
                device.select_weights(wt.data_ptr(), pairs, 0, whi, idx=idx.data_ptr(), cap=hcap, count=cnt.data_ptr())
                device.gather_rows(D, idx.data_ptr(), D=Dh)            # an index of -1 (behind the hits): a zero row
                at = idx.clamp(min=0)
                return [torch.index_select(x, 0, at) for x in (ia, ib, wt)]

            def select(Dm):
                device.join_select(A, B, C0, b, (WC0, WC1), 0, whi, D=Dm, count=cp, hits=hp, ia=sa.data_ptr(), ib=sb.data_ptr(), wt=sw.data_ptr())

            launches = {
                "join": lambda: device.join(A, B, C0, b, D=D, count=cp, ia=ia.data_ptr(), ib=ib.data_ptr(), wt=wt.data_ptr(), wcols=(WC0, WC1)),
                "composed": composed,
                "select": lambda: select(Ds),
                "select_index": lambda: select(unstored),
                "select_counts": lambda: device.join_select(A, B, C0, b, (WC0, WC1), 0, whi, D=none, count=cp, hits=hp, ia=device.SKIP,
                                                            ib=device.SKIP, wt=device.SKIP),
            }
            # the two routes agree before they are timed
            picked = composed()
            select(Ds)
            torch.cuda.synchronize()
            hits, found = int(two[1]), int(cnt[0])
            n = min(hits, hcap)
            assert hits == found and int(two[0]) == pairs, (hits, found)
            assert all(torch.equal(x[:n], y[:n]) for x, y in zip(picked, (sa, sb, sw)))
            k = min(n, 1 << 16)                                   # the first rows go down to the host
            if k:
                assert (device.submatrix(Ds, 0, 0, k, NCOLS).to_words() == device.submatrix(Dh, 0, 0, k, NCOLS).to_words()).all()
            t = timed_together(launches, args.reps)
            res = {"what": "join_select", "NA": N, "NB": N, "b": b, "window": name, "wlo": 0, "whi": whi, "expected_rate": prob, "pairs": pairs,
                   "hits": hits, "observed_rate": round(hits / max(pairs, 1), 6), "pair_capacity": cap, "hit_capacity": hcap, "passes": plan[0],
                   "weigh_lanes": plan[3], "row_lanes": plan[4], "scratch_bytes": plan[6],
                   "composed_output_bytes": cap * (8 * ld + 12), "select_output_bytes": hcap * (8 * ld + 12)}
            res["select_over_composed"] = round(t["select"][0] / t["composed"][0], 3)
            res["select_index_over_composed"] = round(t["select_index"][0] / t["composed"][0], 3)
            res["select_over_join"] = round(t["select"][0] / t["join"][0], 3)
            report(res, t)
            del Dh, Ds, idx, cnt, sa, sb, sw, unstored, launches, picked
        del A, B, D, ia, ib, wt
        torch.cuda.empty_cache()
        L.gf2_trim()
    # a join that the composed route cannot run: more pairs than an int capacity holds
    b, m = big
    N, A, B = pools(b, m)
    expected = m * m << b
    hcap = max(int(2 * p7 * expected), 4096)
    Ds, unstored = device.DMat(hcap, NCOLS), device.DMat.wrap(None, hcap, NCOLS, ld)
    sa, sb, sw = ints(hcap), ints(hcap), ints(hcap)
    plan = device.join_select_plan(N, N, NCOLS, b, (WC0, WC1))

    def select(Dm):
        device.join_select(A, B, C0, b, (WC0, WC1), 0, q7, D=Dm, count=cp, hits=hp, ia=sa.data_ptr(), ib=sb.data_ptr(), wt=sw.data_ptr())

    launches = {
        "join_count": lambda: device.join(A, B, C0, b, D=none, count=cp, ia=device.SKIP, ib=device.SKIP, wt=device.SKIP),
        "select": lambda: select(Ds),
        "select_index": lambda: select(unstored),
        "select_counts": lambda: device.join_select(A, B, C0, b, (WC0, WC1), 0, q7, D=none, count=cp, hits=hp, ia=device.SKIP, ib=device.SKIP,
                                                    wt=device.SKIP),
    }
    select(Ds)
    torch.cuda.synchronize()
    pairs, hits = int(two[0]), int(two[1])
    t = timed_together(launches, max(args.reps // 3, 3))
    res = {"what": "join_select_past_2_to_31", "NA": N, "NB": N, "b": b, "window": "1e-7", "wlo": 0, "whi": q7, "expected_rate": p7, "pairs": pairs,
           "pairs_past_2_to_31": pairs > 1 << 31, "hits": hits, "observed_rate": hits / max(pairs, 1), "hit_capacity": hcap, "passes": plan[0],
           "weigh_lanes": plan[3], "row_lanes": plan[4], "scratch_bytes": plan[6], "composed_output_bytes_needed": pairs * (8 * ld + 12),
           "select_output_bytes": hcap * (8 * ld + 12)}
    res["weigh_pairs_per_ns"] = round(pairs / max(t["select_counts"][0] - t["join_count"][0], 1e-9) / 1e6, 2)
    report(res, t)


if __name__ == "__main__":
    main()
