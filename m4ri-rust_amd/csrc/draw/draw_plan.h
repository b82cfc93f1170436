// draw_plan.h -- how the device draws run, in ONE place: the launchers of gf2_draw.hip launch what this says, draw_host.cpp checks
// the limits and cuts the scratch by it and gf2_draw_plan reports it (the way lf2_plan.h serves the class sort).  Plain host
// arithmetic, no HIP.
#pragma once
#include "../lf2/lf2_plan.h"
#include "philox.h"

constexpr int kDrawThreads = 256;
constexpr int kDrawWaves = kDrawThreads / 64;
// Bernoulli and indices walk their output with a grid of at most kDrawMaxBlocks workgroups; what is left takes further passes
constexpr int kDrawMaxBlocks = 2048;

// ---- Bernoulli: a lane makes one word (rows that are only 8-byte aligned) or two neighbouring ones, stored as 16 bytes
constexpr int kDrawBernoulliCallsMax = 16;
inline int draw_bernoulli_calls(unsigned thr) { return thr ? kDrawBernoulliCallsMax - (__builtin_ctz(thr) >> 1) : 0; }

// ---- subsets
// k <= 64: one wave per subset, kDrawWaves subsets per workgroup; else one workgroup per subset, a lane holds up to
// kDrawSubsetPerLane positions.  Per position the LDS holds (settled value or -1, this round's draw or -1); one int per wave says
// whether it still has an open position.
constexpr int kDrawSubsetMaxK = 1024;
constexpr int kDrawSubsetWaveK = 64;
constexpr int kDrawSubsetPerLane = kDrawSubsetMaxK / kDrawThreads;
constexpr int kDrawSubsetMaxRounds = 64;

struct DrawSubsetPlan {
  int per_group;        // subsets per workgroup; 0: bad k
  long long lds_bytes;  // of the kernel
};

inline DrawSubsetPlan draw_subset_plan(long long k) {
  if (k < 1 || k > kDrawSubsetMaxK) return {0, 0};
  if (k <= kDrawSubsetWaveK) return {kDrawWaves, 8ll * kDrawWaves * kDrawSubsetWaveK + 4 * kDrawWaves};
  return {1, 8ll * kDrawSubsetMaxK + 4 * kDrawWaves};
}

// ---- permutation: the (key, i) pairs, then the class sort's passes over kDrawPermKeyBits (philox.h) key bits.  The scratch is the
// sort's own: two pair buffers, digit counts, chunk sums
inline Lf2Plan draw_perm_plan(long long n) { return lf2_plan(n, 0, kDrawPermKeyBits); }
