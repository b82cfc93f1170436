// unique_plan.h -- how the row sort on a column range and the duplicate removal run, in ONE place: the launchers of gf2_unique.hip
// launch what this says, unique_host.cpp cuts the scratch by it and gf2_sort_rows_plan reports it (the way lf2_plan.h serves the class
// sort, whose passes and work space this module uses as they are).  Plain host arithmetic, no HIP.
#pragma once
#include "../lf2/lf2_plan.h"
#include "../weight/weight_plan.h"

// ---- the sort: a chain of stable sorts, one per WINDOW of the range, least significant window first
// The range [c0, c1) is cut from c0 upward into windows of kUniqueWindowBits columns; the last window takes what is left.  A window is
// sorted by the passes of the class sort (lf2_plan.h: kLf2DigitBits bits each) on pairs (the window's bits of a row, the row) that the
// rekey kernel writes in the order the windows below it have left.  24 = 3 * 8: every pass of every window but the last is a full
// one, and the passes of all windows together are ceil((c1 - c0) / 8), as many as one sort of a key that wide would take.
constexpr int kUniqueWindowBits = 24;
static_assert(kUniqueWindowBits % kLf2DigitBits == 0 && kUniqueWindowBits <= kLf2MaxB, "whole passes, and a key that gf2_row_key reads");
constexpr int kUniqueLaunchesPerPass = 5;  // gf2k_lf2_sort_pass: count, three of the scan, scatter

// ---- the heads
// A workgroup of kUniqueThreads lanes owns a run of kUniqueRunRows consecutive sorted positions.
constexpr int kUniqueThreads = 256;
constexpr int kUniqueWaves = kUniqueThreads / 64;
constexpr int kUniqueRunItems = 4;
constexpr int kUniqueRunRows = kUniqueThreads * kUniqueRunItems;
constexpr int kUniqueHeadLaunches = 3;  // flags and run summaries, the carries, the fill

// the words of a row that hold a column of [c0, c1): [first, end); an empty range holds no word: both are 0
constexpr long long unique_first_word(long long c0, long long c1) { return c0 < c1 ? c0 >> 6 : 0; }
constexpr long long unique_end_word(long long c0, long long c1) { return c0 < c1 ? ((c1 - 1) >> 6) + 1 : 0; }

// window `win` of the range: its first column and its bits
constexpr int unique_window_c0(int c0, int win) { return c0 + kUniqueWindowBits * win; }
constexpr int unique_window_bits(int c0, int c1, int win) {
  return c1 - unique_window_c0(c0, win) < kUniqueWindowBits ? c1 - unique_window_c0(c0, win) : kUniqueWindowBits;
}

struct UniquePlan {
  int windows;               // ceil((c1 - c0) / 24), 0 for an empty range; -1: bad shape
  int passes;                // radix passes of all windows: ceil((c1 - c0) / 8)
  int sort_launches;         // gf2_sort_rows_dev without head: a rekey and 5 per pass for every window; 1 (the iota) for an empty range
  int unique_launches;       // gf2_unique_rows_dev with cap > 0: the sort, the heads, rep and flags, 3 of the selection
  long long runs;            // runs of the head kernels
  long long work_bytes;      // the work space of the passes: two pair buffers, digit counts, chunk sums (lf2_plan: sort_scratch)
  long long carry_bytes;     // one int32 per run
  long long order_bytes;     // the sorted order of gf2_unique_rows_dev
  long long block_bytes;     // the block counts of the selection
  long long sort_scratch;    // gf2_sort_rows_dev: work, carries
  long long unique_scratch;  // gf2_unique_rows_dev: work (head and the flags lie in its first pair buffer once the sort is done), carries, order, block counts
};

inline UniquePlan unique_plan(long long nrows, long long ncols, long long c0, long long c1) {
  UniquePlan p = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (nrows < 0 || nrows > 0x7FFFFFFFll || ncols < 0 || ncols > 0x7FFFFFFFll || c0 < 0 || c0 > c1 || c1 > ncols) return p;
  const long long width = c1 - c0;
  p.windows = (int)((width + kUniqueWindowBits - 1) / kUniqueWindowBits);
  p.passes = (int)((width + kLf2DigitBits - 1) / kLf2DigitBits);
  p.sort_launches = p.windows ? p.windows + kUniqueLaunchesPerPass * p.passes : 1;
  p.unique_launches = p.sort_launches + kUniqueHeadLaunches + 1 + 3;
  p.runs = (nrows + kUniqueRunRows - 1) / kUniqueRunRows;
  p.work_bytes = lf2_plan(nrows, 0, kUniqueWindowBits).sort_scratch;
  p.carry_bytes = lf2_align16(4 * p.runs);
  p.order_bytes = lf2_align16(4 * nrows);
  p.block_bytes = lf2_align16(4 * ((nrows + kWeightSelectBlock - 1) / kWeightSelectBlock));
  p.sort_scratch = p.work_bytes + p.carry_bytes;
  p.unique_scratch = p.work_bytes + p.carry_bytes + p.order_bytes + p.block_bytes;
  return p;
}

// the scratch of a call, from `base` on.  head and flags (gf2_unique_rows_dev) are the two halves of the first pair buffer: 8 nrows
// bytes that the sort no longer needs when the heads are taken
struct UniqueWork {
  void *work;  // lf2_sort_work cuts it
  int *carry, *order, *blocks, *head, *flags;
};
inline UniqueWork unique_work(void *base, const UniquePlan &p, long long nrows) {
  char *at = static_cast<char *>(base);
  int *pairs0 = reinterpret_cast<int *>(at);
  return {at,
          reinterpret_cast<int *>(at + p.work_bytes),
          reinterpret_cast<int *>(at + p.work_bytes + p.carry_bytes),
          reinterpret_cast<int *>(at + p.work_bytes + p.carry_bytes + p.order_bytes),
          pairs0,
          pairs0 + nrows};
}
