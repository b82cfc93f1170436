// bkw_plan.h -- how an LF1 round runs, in ONE place: the launchers of gf2_bkw.hip launch what this says and gf2_lf1_plan reports it
// (the way wht_plan.h serves the tally).  Plain host arithmetic, no HIP.
#pragma once

constexpr int kLf1MaxB = 30;  // a table of 2^30 int32 = 4 GiB at the most; the key spans at most two words of a row

// ---- class firsts
// Up to kLf1LdsLevels the 2^b minima fit a workgroup's LDS (64 KiB: two workgroups per compute unit); above, a row goes straight to
// the table in global memory.  A workgroup of the LDS variant pays up to 2^b global atomics for its flush, so it is not started for
// fewer than kLf1FirstGroupRows rows.  The geometry is the tally's (wht_plan.h); DESIGN.md section 7.11 has what was measured.
constexpr int kLf1FirstThreads = 512;
constexpr int kLf1LdsLevels = 14;
constexpr int kLf1FirstGroupRows = 4096;
constexpr int kLf1FirstLdsGroups = 512;      // workgroups at the most, LDS variant (two per compute unit)
constexpr int kLf1FirstGlobalGroups = 2048;  // ... and of the global variant

inline int lf1_first_variant(int b) { return b <= kLf1LdsLevels ? 0 : 1; }

inline long long lf1_first_groups(long long nrows, int variant) {
  const bool lds = variant == 0;
  const long long per = lds ? kLf1FirstGroupRows : kLf1FirstThreads, cap = lds ? kLf1FirstLdsGroups : kLf1FirstGlobalGroups;
  const long long g = (nrows + per - 1) / per;
  return g < 1 ? 1 : g > cap ? cap : g;
}

// ---- count, scan, scatter
// A workgroup of kLf1Threads lanes covers a fixed run of consecutive rows: lane t ranks the rows t, t + 256, ... of the run, so a wave
// looks at 64 consecutive rows at a time and the ranks of the survivors follow from a ballot.  Rows of up to kLf1NarrowWords words
// (the LPN shapes) are ranked four per lane and moved by a lane per 16-byte piece: one lane up to kLf1PieceWords words, two above
// (at four words, one lane per row took 1.4 times as long).  Wider rows are ranked one per lane and moved by 8
// or 64 lanes each, as the weight kernels cut it.
constexpr int kLf1Threads = 256;
constexpr int kLf1NarrowWords = 4;
constexpr int kLf1PieceWords = 2;   // 16 bytes
constexpr int kLf1MidWords = 64;
constexpr int kLf1NarrowItems = 4;  // rows per lane of the narrow kernels
constexpr int kLf1ScanItems = 4;    // block counts per lane and round of the scan kernel
constexpr int kLf1ScanChunk = kLf1Threads * kLf1ScanItems;

struct Lf1Plan {
  int variant;        // of the class-first kernel: 0 LDS table, 1 global atomics; -1: bad shape
  int lanes;          // lanes per row of the scatter kernel: 1, 2, 8 or 64
  int rows;           // rows a workgroup of the count / scatter kernels covers
  long long blocks;   // such workgroups
  long long scratch;  // bytes: one int per block
};

inline Lf1Plan lf1_plan(long long nrows, long long ncols, int b) {
  if (nrows < 0 || ncols < 0 || b < 0 || b > kLf1MaxB) return {-1, 0, 0, 0, 0};
  const long long nw = (ncols + 63) >> 6;
  const int lanes = nw <= kLf1PieceWords ? 1 : nw <= kLf1NarrowWords ? 2 : nw <= kLf1MidWords ? 8 : 64;
  const int rows = kLf1Threads * (nw <= kLf1NarrowWords ? kLf1NarrowItems : 1);
  const long long blocks = (nrows + rows - 1) / rows;
  return {lf1_first_variant(b), lanes, rows, blocks, 4 * blocks};
}
