// wht_plan.h -- how a Walsh-Hadamard transform of 2^k int32, the LPN tally in front of it and the minimum behind it run, in ONE place:
// the launchers of gf2_wht.hip launch what this says and gf2_wht_plan reports it (the way weight_plan.h serves the weights).  Plain
// host arithmetic, no HIP.
#pragma once

constexpr int kWhtMaxK = 30;      // 2^30 int32 = 4 GiB: the largest array (every index fits an int32)
constexpr int kWhtMaxPasses = 8;  // what gf2_wht_plan can report; the plan below needs 5 at k = 30

// ---- the transform
// The first pass takes a contiguous tile of 2^kWhtLowLevels elements per workgroup (levels 0 .. 11: in the 16-byte vector, across a
// lane's four vectors, across the lanes of a wave, across the four waves through LDS).  A later pass takes 2^b rows that lie
// 2^first elements apart, a 16-byte column of them per lane, and butterflies across the rows in registers: b <= kWhtHighMaxLevels
// (32 vectors = 128 registers per lane).  The levels above the tile are spread evenly over as few such passes as hold them.
constexpr int kWhtThreads = 256;
constexpr int kWhtLowLevels = 12;
constexpr int kWhtHighMaxLevels = 5;
constexpr int kWhtLdsBytes = 4 << kWhtLowLevels;  // the tile, once: 16 KiB

struct WhtPlan {
  int passes;                    // -1: bad k
  int first[kWhtMaxPasses + 1];  // pass p covers the levels [first[p], first[p + 1]); entries from `passes` on are k
};

inline WhtPlan wht_plan(int k) {
  WhtPlan p;
  p.passes = (k < 0 || k > kWhtMaxK) ? -1 : 0;
  for (int i = 0; i <= kWhtMaxPasses; ++i) p.first[i] = k;
  if (p.passes < 0 || k == 0) return p;
  const int low = k < kWhtLowLevels ? k : kWhtLowLevels;
  p.first[p.passes++] = 0;
  const int high = k - low;
  const int n = (high + kWhtHighMaxLevels - 1) / kWhtHighMaxLevels;
  int level = low;
  for (int i = 0; i < n; ++i) {
    p.first[p.passes++] = level;
    level += high / n + (i < high % n ? 1 : 0);
  }
  return p;
}

// ---- the tally
// Up to kWhtTallyLdsLevels the 2^k counters fit a workgroup's LDS (64 KiB: two workgroups per compute unit); above, every row is one
// global atomic.  A workgroup of the LDS variant pays 2^k global atomics for its flush at the most, so it is not started for fewer
// than kWhtTallyGroupRows rows.
constexpr int kWhtTallyThreads = 512;
constexpr int kWhtTallyLdsLevels = 14;
constexpr int kWhtTallyGroupRows = 4096;
constexpr int kWhtTallyLdsGroups = 512;      // workgroups at the most, LDS variant (two per compute unit)
constexpr int kWhtTallyGlobalGroups = 2048;  // ... and of the global variant

inline int wht_tally_variant(int k) { return k <= kWhtTallyLdsLevels ? 0 : 1; }

inline long long wht_tally_groups(long long nrows, int k) {
  const bool lds = wht_tally_variant(k) == 0;
  const long long per = lds ? kWhtTallyGroupRows : kWhtTallyThreads, cap = lds ? kWhtTallyLdsGroups : kWhtTallyGlobalGroups;
  const long long g = (nrows + per - 1) / per;
  return g < 1 ? 1 : g > cap ? cap : g;
}

// ---- the minimum: blocks of kWhtMinBlock values, at most kWhtMinGroups workgroups (a grid-stride loop over the blocks); the
// (value, index) pair of each workgroup is the call's scratch
constexpr int kWhtMinItems = 4;
constexpr int kWhtMinBlock = kWhtThreads * kWhtMinItems;
constexpr int kWhtMinGroups = 1024;

inline long long wht_min_groups(long long n) {
  const long long g = (n + kWhtMinBlock - 1) / kWhtMinBlock;
  return g < 1 ? 1 : g > kWhtMinGroups ? kWhtMinGroups : g;
}
inline long long wht_min_scratch(long long n) { return 8 * wht_min_groups(n); }
