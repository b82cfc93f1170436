// join_rows_plan.h -- how the grouping of a pool by class and the join of two pools on a column range of any width run, in ONE place:
// the launchers of gf2_join_rows.hip launch what this says, join_rows_host.cpp cuts the scratch by it and gf2_join_rows_plan reports
// it (the way find_plan.h serves the lookup, whose table and kernels this module uses as they are, and lf2_plan.h the class sort,
// whose passes it uses).  Below the plan: the pure index arithmetic of the scatter -- the text that the kernels and the CPU tests
// (tests/join_rows_emu.cpp) share.  Plain arithmetic in constexpr functions, which compile for host and device alike; no HIP.
#pragma once
#include <stdint.h>

#include "../find/find_plan.h"
#include "../lf2/lf2_plan.h"

// ---- the kernels
// A workgroup has kJoinRowsThreads lanes.  The pair, start and head kernels take a row or a sorted position per lane.  The sum and
// offset kernels own a run of kJoinRowsRunRows consecutive rows of A, kJoinRowsRunItems consecutive ones per lane.  A workgroup of
// the scatter owns a CHUNK of kJoinRowsChunk consecutive OUTPUTS and stages the offsets of up to kJoinRowsChunk rows of A in LDS (16
// KiB); a chunk whose rows lie further apart (long stretches of rows without a partner) bisects the offsets in global memory.
constexpr int kJoinRowsThreads = 256;
constexpr int kJoinRowsWaves = kJoinRowsThreads / 64;
constexpr int kJoinRowsRunItems = 4;
constexpr int kJoinRowsRunRows = kJoinRowsThreads * kJoinRowsRunItems;
constexpr int kJoinRowsChunk = 2048;

// ---- the grouping: a stable sort of the pairs (rep(j), j) by rep, so by (rep, row)
// rep(j) < NB has bits(NB - 1) bits, which the passes of the class sort (lf2_plan.h: kLf2DigitBits bits each) sort in one window
// while a key of the sort holds them (kLf2MaxB = 30 bits); the 31 bits of a pool of more than 2^30 rows go in two windows, the lower
// kJoinRowsLowBits = 24 bits in three full passes and the rest in a fourth, chained as the windows of unique_plan.h are.
constexpr int kJoinRowsLowBits = 24;
static_assert(kJoinRowsLowBits % kLf2DigitBits == 0 && kJoinRowsLowBits <= kLf2MaxB, "whole passes, and a key of the sort");
constexpr int kJoinRowsLaunchesPerPass = 5;  // gf2k_lf2_sort_pass: count, three of the scan, scatter

// the bits of the largest row index of a pool of n rows: 0 for n <= 1
constexpr int join_rows_index_bits(long long n) {
  int b = 0;
  while (n > 1 && ((n - 1) >> b) != 0) ++b;
  return b;
}
constexpr int join_rows_windows(int bits) { return bits == 0 ? 0 : bits <= kLf2MaxB ? 1 : 2; }
// window `win` of a key of `bits` bits: its first bit and its width
constexpr int join_rows_window_shift(int bits, int win) { return join_rows_windows(bits) == 2 ? kJoinRowsLowBits * win : 0; }
constexpr int join_rows_window_bits(int bits, int win) {
  return join_rows_windows(bits) == 2 ? (win == 0 ? kJoinRowsLowBits : bits - kJoinRowsLowBits) : bits;
}

// ---- the scatter's index arithmetic
// offs[i] = the outputs of the rows of A before row i (ascending; equal where a row has no partner).  The row of output t is the
// LARGEST q of [lo, hi) with offs[q] <= t; offs[lo] <= t is the caller's.  A row without outputs is never the answer: the row behind
// it has the same offset.  Reads offs[lo + 1 .. hi) alone
constexpr long long join_rows_find_row(const long long *offs, long long lo, long long hi, long long t) {
  while (hi - lo > 1) {  // offs[lo] <= t, and hi is the end or offs[hi] > t
    const long long mid = lo + ((hi - lo) >> 1);
    if (offs[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// the outputs [*t0, *t1) of chunk `chunk` when `limit` = min(count, capacity) outputs are written: false where the chunk has none
constexpr bool join_rows_chunk_outputs(long long chunk, long long limit, long long *t0, long long *t1) {
  *t0 = chunk * kJoinRowsChunk;
  *t1 = *t0 + kJoinRowsChunk < limit ? *t0 + kJoinRowsChunk : limit;
  return *t0 < limit;
}

// ---- the plan
struct JoinRowsPlan {
  int passes;              // radix passes of the grouping: ceil(bits(NB - 1) / 8), 0 for NB <= 1; -1: bad shape or range
  int bits, windows;       // bits(NB - 1) and the windows they are sorted in: 0, 1 or 2
  int wave;                // the form of the table's kernels (find_plan.h): 0 a lane per row, 1 a wave per row
  int lanes;               // lanes per row of the scatter (lf2_plan.h: by the row width)
  int group_launches;      // gf2_group_rows_dev with head == NULL (two more with head); 0 for NB == 0
  int count_launches;      // gf2_join_rows_dev, the count-only call; 0 where NA == 0 or NB == 0
  int join_launches;       // gf2_join_rows_dev with a capacity and something to write
  long long slots;         // of the table over B
  long long table_bytes;   // the table (find_plan: scratch), to 16 bytes
  long long rep_bytes;     // rep of B; as much again for the sorted order of B and for the class starts
  long long work_bytes;    // the work space of the passes: two pair buffers, digit counts, chunk sums (lf2_plan: sort_scratch)
  long long idx_bytes;     // idx of A; as much again for mult
  long long offs_bytes;    // the 64-bit offsets of the rows of A
  long long runs;          // runs of A
  long long sums_bytes;    // a 64-bit sum per run
  long long group_scratch, join_scratch;
};

inline JoinRowsPlan join_rows_plan(long long nrows_a, long long nrows_b, long long ncols, long long c0, long long c1) {
  JoinRowsPlan p = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const FindPlan f = find_plan(nrows_a, nrows_b, ncols, c0, c1);
  if (f.slots < 0) return p;
  p.bits = join_rows_index_bits(nrows_b);
  p.windows = join_rows_windows(p.bits);
  p.passes = (p.bits + kLf2DigitBits - 1) / kLf2DigitBits;
  p.wave = f.wave;
  p.lanes = lf2_plan(nrows_a, ncols, 0).lanes;
  const int sort_launches = p.passes ? p.windows + kJoinRowsLaunchesPerPass * p.passes : 1;  // pairs per window and the passes, or the iota
  p.group_launches = nrows_b > 0 ? kFindLaunches + sort_launches : 0;
  p.count_launches = nrows_a > 0 && nrows_b > 0 ? kFindLaunches + 2 : 0;                         // lookup of A, run sums, their scan
  p.join_launches = p.count_launches ? p.count_launches + 1 + p.group_launches + 1 + 1 : 0;     // offsets, the grouping, starts, scatter
  p.slots = f.slots;
  p.table_bytes = lf2_align16(f.scratch);
  p.rep_bytes = lf2_align16(4 * nrows_b);
  p.work_bytes = lf2_plan(nrows_b, 0, kJoinRowsLowBits).sort_scratch;
  p.idx_bytes = lf2_align16(4 * nrows_a);
  p.offs_bytes = lf2_align16(8 * nrows_a);
  p.runs = (nrows_a + kJoinRowsRunRows - 1) / kJoinRowsRunRows;
  p.sums_bytes = lf2_align16(8 * p.runs);
  p.group_scratch = p.table_bytes + 2 * p.rep_bytes + p.work_bytes;  // table, rep, starts, work
  p.join_scratch = p.table_bytes + 3 * p.rep_bytes + p.work_bytes + 2 * p.idx_bytes + p.offs_bytes + p.sums_bytes;
  return p;
}

// the scratch of a call, from `base` on.  gf2_group_rows_dev uses table, rep, start and work (its order is the caller's)
struct JoinRowsWork {
  void *table;
  int *rep, *start, *order;
  void *work;  // lf2_sort_work cuts it
  int *idx, *mult;
  long long *offs, *sums;
};
inline JoinRowsWork join_rows_work(void *base, const JoinRowsPlan &p, bool join) {
  char *at = static_cast<char *>(base);
  JoinRowsWork w = {};
  w.table = at;
  at += p.table_bytes;
  w.rep = reinterpret_cast<int *>(at);
  w.start = reinterpret_cast<int *>(at + p.rep_bytes);
  at += 2 * p.rep_bytes;
  w.work = at;
  at += p.work_bytes;
  if (!join) return w;
  w.order = reinterpret_cast<int *>(at);
  at += p.rep_bytes;
  w.idx = reinterpret_cast<int *>(at);
  w.mult = reinterpret_cast<int *>(at + p.idx_bytes);
  at += 2 * p.idx_bytes;
  w.offs = reinterpret_cast<long long *>(at);
  w.sums = reinterpret_cast<long long *>(at + p.offs_bytes);
  return w;
}
