// join_plan.h -- how the join of two pools runs, in ONE place: the launchers of gf2_join.hip launch what this says, join_host.cpp cuts
// the scratch by it and gf2_join_plan reports it (the way lf2_plan.h serves LF2, whose sort and lane thresholds it takes over).
// Plain host arithmetic, no HIP.
#pragma once
#include "../lf2/lf2_plan.h"

constexpr int kJoinMaxB = kLf2MaxB;
constexpr int kJoinThreads = kLf2Threads;  // the block sums below count on the waves of the LF2 kernels
constexpr int kJoinWaves = kJoinThreads / 64;
// A workgroup owns a run of kJoinRunRows consecutive sorted positions of A, kJoinRunItems consecutive ones per lane, and stages up to
// kJoinSpanKeys sorted keys of B in LDS: the positions of B that the run's keys can meet.  A longer span is bisected in global memory.
constexpr int kJoinRunItems = 4;
constexpr int kJoinRunRows = kJoinThreads * kJoinRunItems;
constexpr int kJoinSpanKeys = 4096;
// LDS of the scatter kernel, the larger of the two: sums before every position, the first partner of every position, the staged
// span, the span's ends and the waves' sums.  28 KiB and a few bytes: five workgroups per CU by LDS
constexpr int kJoinLds = 8 * kJoinRunRows + 4 * kJoinRunRows + 4 * kJoinSpanKeys + 8 + 8 * kJoinWaves;

struct JoinPlan {
  int passes;            // of either sort: ceil(b / 8), 0 for b == 0; -1: bad shape
  int lanes;             // lanes per row of the scatter
  long long runs;        // runs of A
  long long sort_bytes;  // the sort's work space, shared by the two sorts (they follow each other on the stream)
  long long order_a;     // order of A (and as much again for its sorted keys)
  long long order_b;     // ... of B
  long long scratch;     // all of it: sort work space, order and keys of A, of B, run sums
};

inline JoinPlan join_plan(long long nrows_a, long long nrows_b, long long ncols, int b) {
  const Lf2Plan pa = lf2_plan(nrows_a, ncols, b), pb = lf2_plan(nrows_b, ncols, b);
  if (pa.passes < 0 || pb.passes < 0) return {-1, 0, 0, 0, 0, 0, 0};
  JoinPlan p;
  p.passes = pa.passes;
  p.lanes = pa.lanes;
  p.runs = (nrows_a + kJoinRunRows - 1) / kJoinRunRows;
  p.sort_bytes = p.passes ? (pa.sort_scratch > pb.sort_scratch ? pa.sort_scratch : pb.sort_scratch) : 0;
  p.order_a = pa.order_bytes;
  p.order_b = pb.order_bytes;
  p.scratch = p.sort_bytes + 2 * p.order_a + 2 * p.order_b + lf2_align16(8 * p.runs);
  return p;
}

// ---- the weight-filtered join (gf2_join_select_dev; kernels: gf2_join_select.inc)
// LDS of its scatter kernel: the join's, and two rows of the waves' hits of a round
constexpr int kJoinSelectLds = kJoinLds + 2 * 4 * kJoinWaves;

struct JoinSelectPlan {
  JoinPlan join;        // sorts, runs, lanes per row of the row store and the join's scratch, as they are
  int weigh_lanes;      // lanes per pair of the weigh pass: by the words of a row that hold a column of the weight range
  int round_outputs;    // outputs per round of the scatter: one per group of join.lanes lanes
  long long hit_bytes;  // the hit sums: one array of a long long per run, twice (the scan turns one into offsets, the other stays)
  long long scratch;    // all of it: the join's scratch, then the hit sums
};

// wc0 <= wc1: the weight range, checked by the caller (an empty one holds no word)
inline JoinSelectPlan join_select_plan(long long nrows_a, long long nrows_b, long long ncols, int b, long long wc0, long long wc1) {
  JoinSelectPlan p;
  p.join = join_plan(nrows_a, nrows_b, ncols, b);
  p.weigh_lanes = p.round_outputs = 0;
  p.hit_bytes = p.scratch = 0;
  if (p.join.passes < 0) return p;
  const long long words = wc0 < wc1 ? ((wc1 - 1) >> 6) - (wc0 >> 6) + 1 : 0;
  p.weigh_lanes = words <= kLf2PieceWords ? 1 : words <= kLf2NarrowWords ? 2 : words <= kLf2MidWords ? 8 : 64;
  p.round_outputs = kJoinThreads / p.join.lanes;
  p.hit_bytes = 2 * lf2_align16(8 * p.join.runs);
  p.scratch = p.join.scratch + p.hit_bytes;
  return p;
}
