// weight_plan.h -- which kernel a Hamming-weight call runs on and with what geometry, in ONE place: the launchers of gf2_weight.hip
// launch what this says and gf2_weights_plan reports it (the way gather_plan.h serves the column gather).  Plain host arithmetic, no
// HIP.
#pragma once

// ---- row weights and the total
constexpr int kWeightThreads = 256;       // every row / total / select kernel
constexpr int kWeightNarrowWords = 4;     // rows of up to this many words: one lane per row (the word-level kernel)
constexpr int kWeightMidWords = 64;       // up to this many: 8 lanes per row; above: a wave per row
constexpr int kWeightTotalBlocks = 1024;  // workgroups of the total at the most: one 64-bit atomic add each

// ---- column weights (gf2_weight_cols_kernel)
// A lane owns a SLICE of two word columns (16 bytes of every row) and walks down the rows of its band, a row every `wy`.  It adds
// the words it loads into six bit-sliced counter planes per word (1, 2, 4 from a carry-save tree over 8 rows; 8, 16, 32 by a ripple
// of the tree's carry), which hold 63 at the most: after kWeightFlushRows rows the planes are emptied into the workgroup's LDS
// counters, one integer per column.
constexpr int kWeightColThreads = 128;   // two waves: wx lanes across the slices of a row, wy = 128 / wx rows per pass
constexpr int kWeightColMaxWx = 64;      // 64 slices = 128 words = 8192 columns per workgroup; 32 KiB of LDS counters
constexpr int kWeightCsaRows = 8;        // rows per carry-save tree
constexpr int kWeightPlanes = 6;         // counter planes per word
constexpr int kWeightFlushRows = 56;     // 7 trees; < 2^kWeightPlanes
constexpr int kWeightMinLaneRows = 64;   // a band is not cut below this many rows per lane: more bands than that buy nothing
constexpr int kWeightMaxGroups = 1024;   // workgroups aimed at (4 per CU): bands = this / column groups at the most
static_assert(kWeightFlushRows % kWeightCsaRows == 0 && kWeightFlushRows < (1 << kWeightPlanes), "the planes must hold a flush period");
static_assert(kWeightMinLaneRows % kWeightCsaRows == 0, "bands are whole trees");

struct WeightRowsPlan {
  int variant;  // 0: a lane per row, 1: several lanes per row; -1: bad shape
  int lanes;    // lanes per row: 1, 8 or 64
  int rows;     // rows per workgroup and pass of the row loop
};

inline WeightRowsPlan weight_rows_plan(long long nrows, long long ncols) {
  if (nrows < 0 || ncols < 0) return {-1, 0, 0};
  const long long nw = (ncols + 63) >> 6;
  const int lanes = nw <= kWeightNarrowWords ? 1 : nw <= kWeightMidWords ? 8 : 64;
  return {lanes == 1 ? 0 : 1, lanes, kWeightThreads / lanes};
}

struct WeightColsPlan {
  int variant;          // 0: one band, stored straight into `weights`; 1: per-band partial sums in stream scratch and a fold launch
  int wx, wy;           // lanes across a row's slices, rows per pass
  long long groups;     // column groups of wx slices (grid.x)
  long long bands;      // bands of rows (grid.y)
  long long lane_rows;  // rows a lane takes in a band (a multiple of kWeightCsaRows); band rows = lane_rows * wy
  long long scratch;    // bytes
};

inline WeightColsPlan weight_cols_plan(long long nrows, long long ncols) {
  if (nrows < 0 || ncols < 0) return {-1, 0, 0, 0, 0, 0, 0};
  const long long slices = (((ncols + 63) >> 6) + 1) >> 1;
  int wx = 1;
  while (wx < slices && wx < kWeightColMaxWx) wx <<= 1;
  const int wy = kWeightColThreads / wx;
  const long long groups = slices ? (slices + wx - 1) / wx : 1;
  const long long max_bands = groups >= kWeightMaxGroups ? 1 : kWeightMaxGroups / groups;
  const long long passes = (nrows + wy - 1) / wy;  // rows the busiest lane would take with one band
  long long lane_rows = (passes + max_bands - 1) / max_bands;
  if (lane_rows < kWeightMinLaneRows) lane_rows = kWeightMinLaneRows;
  lane_rows = (lane_rows + kWeightCsaRows - 1) / kWeightCsaRows * kWeightCsaRows;
  long long bands = (passes + lane_rows - 1) / lane_rows;
  if (bands < 1) bands = 1;
  return {bands > 1 ? 1 : 0, wx, wy, groups, bands, lane_rows, bands > 1 ? 4 * bands * ncols : 0};
}

struct WeightTotalPlan {
  int variant;  // 0, 1, 2: 1, 8, 64 lanes per row; -1: bad shape
  int lanes;
  int rows;  // rows per workgroup and pass
};

inline WeightTotalPlan weight_total_plan(long long nrows, long long ncols) {
  const WeightRowsPlan r = weight_rows_plan(nrows, ncols);
  if (r.variant < 0) return {-1, 0, 0};
  return {r.lanes == 1 ? 0 : r.lanes == 8 ? 1 : 2, r.lanes, r.rows};
}

// select: blocks of this many weights; the per-block match counts (one int each) are the call's scratch
constexpr int kWeightSelectItems = 4;
constexpr int kWeightSelectBlock = kWeightThreads * kWeightSelectItems;
