// sums_plan.h -- the order of the subset sums and how they run, in ONE place (include/m4ri_hip_sums.h).
//
// The order: the combinatorial number system.  A subset c_1 < ... < c_p of {0, 1, ...} has the rank C(c_1, 1) + ... + C(c_p, p); by
// ascending rank the subsets are in colexicographic order, and the rank does not depend on the size of the ground set.  The binomial,
// rank, unrank and advance routines below are plain C++ and the same text is compiled for the host (sums_host.cpp: gf2_subset_count,
// gf2_subset_rank, gf2_subset_unrank) and for the device (gf2_sums.hip), the way draw/philox.h serves the draws;
// tests/test_sums_helpers_cpu.py runs that text under the host compiler's sanitizers.
//
// The plan: the launchers of gf2_sums.hip launch what sums_plan says and gf2_subset_sums_plan reports it (the way join_plan.h serves
// the join, whose lane thresholds it takes over).  Plain host arithmetic, no HIP.
#pragma once
#include <stdint.h>

#include "../lf2/lf2_plan.h"

#if defined(__HIPCC__)
#define GF2_SUMS_FN __host__ __device__ __forceinline__
#else
#define GF2_SUMS_FN inline
#endif

constexpr int kSumsMaxP = 4;
constexpr unsigned kSumsNone = 0xFFFFFFFFu;                // c_i of a level above p: no carry ever reaches it
constexpr unsigned long long kSumsMaxCount = 1ull << 62;   // C(n, p) may not pass this

// the largest c whose C(c, i) stays below 2^63: every binomial that the bisection of sums_unrank forms fits 64 bits
GF2_SUMS_FN unsigned sums_max_c(int i) { return i >= 4 ? 121977u : i == 3 ? 3810779u : 0xFFFFFFFEu; }

// C(c, i) for 1 <= i <= 4 and c <= sums_max_c(i); 0 for c < i.  Every product is divided before it can pass 64 bits: with v = C(c, j),
// v (c - j) = (j + 1) C(c, j + 1), and (v % (j + 1)) (c - j) is a multiple of j + 1 because the whole is and (v / (j + 1)) (j + 1) (c - j) is
GF2_SUMS_FN unsigned long long sums_binomial(unsigned c, int i) {
  unsigned long long v = c;
  if (i <= 1) return v;
  if (c < (unsigned)i) return 0;
  v = v * (c - 1) / 2;
  if (i == 2) return v;
  v = (v / 3) * (c - 2) + (v % 3) * (c - 2) / 3;
  if (i == 3) return v;
  return (v / 4) * (c - 3) + (v % 4) * (c - 3) / 4;
}

// the rank of c_1 < ... < c_p (c[i - 1] = c_i); the caller has checked the order and C(c_p + 1, p) <= 2^62
GF2_SUMS_FN unsigned long long sums_rank(const unsigned c[4], int p) {
  unsigned long long r = 0;
#pragma unroll
  for (int i = 1; i <= kSumsMaxP; ++i)
    if (i <= p) r += sums_binomial(c[i - 1], i);
  return r;
}

// c <- the subset of {0 .. n - 1} of size p with the largest rank that is <= rank, level by level from the top: c_i is the largest
// value below c_(i+1) (below n for i = p) with C(c_i, i) <= what is left, found by bisection.  n >= p.  The levels above p get
// kSumsNone.  -> what is left at the end: 0 exactly when rank < C(n, p), that is when c is the subset of that rank
GF2_SUMS_FN unsigned long long sums_unrank(unsigned long long rank, int p, unsigned n, unsigned c[4]) {
  unsigned top = n;  // c_i < top
#pragma unroll
  for (int i = kSumsMaxP; i >= 1; --i) {
    if (i > p) {
      c[i - 1] = kSumsNone;
      continue;
    }
    unsigned lo = (unsigned)i - 1, hi = top - 1;  // C(lo, i) = 0 <= rank
    if (hi > sums_max_c(i)) hi = sums_max_c(i);
    while (lo < hi) {
      const unsigned mid = lo + (hi - lo + 1) / 2;
      if (sums_binomial(mid, i) <= rank)
        lo = mid;
      else
        hi = mid - 1;
    }
    c[i - 1] = lo;
    rank -= sums_binomial(lo, i);
    top = lo;
  }
  return rank;
}

// c <- the subset `stride` ranks further on, by the carry chain of the order: the subsets that share c_2 .. c_p are a block of c_2
// consecutive ranks, c_1 = 0 .. c_2 - 1; past its end the rest of the stride goes into the block of c_2 + 1, and where c_2 reaches
// c_3 the next block is the first one of c_3 + 1 (c_2 = 1), and so on upwards.  stride <= 2^30; the levels above p hold kSumsNone.
// -> whether a level above the first moved (the XOR of the rows c_2 .. c_p has to be redone)
GF2_SUMS_FN bool sums_advance(unsigned c[4], unsigned stride) {
  unsigned c1 = c[0] + stride;  // c_1 < 2^31: no wrap
  bool carried = false;
  while (c1 >= c[1]) {
    c1 -= c[1];
    carried = true;
    if (++c[1] == c[2]) {
      c[1] = 1;
      if (++c[2] == c[3]) {
        c[2] = 2;
        ++c[3];
      }
    }
  }
  c[0] = c1;
  return carried;
}

// C(n, p) as gf2_subset_count returns it: 0 for n < p, -1 for a p outside 1 .. 4 or a value past 2^62
inline long long sums_count(long long n, int p) {
  if (p < 1 || p > kSumsMaxP) return -1;
  if (n < p) return 0;
  if (n > (long long)sums_max_c(p)) return -1;
  const unsigned long long v = sums_binomial((unsigned)n, p);
  return v > kSumsMaxCount ? -1 : (long long)v;
}

// ---- the plan
// A workgroup of kSumsThreads lanes takes `ranks` consecutive ranks.  `lanes` lanes share a row (1, 2, 8 or 64 by the row width, the
// thresholds of the LF2 / join scatters); group g of the kSumsThreads / lanes groups takes the ranks g, g + groups, ... of the
// workgroup, so that a wave writes consecutive rows.  S (and base) are copied into LDS when n + 1 rows fit kSumsLdsBytes -- two
// workgroups per CU of the 160 KiB, with room to spare -- and are read from global memory, through L2, otherwise.
constexpr int kSumsThreads = 256;
constexpr int kSumsLdsBytes = 64 * 1024;
constexpr int kSumsCachedUnits = 4;  // 16-byte pieces of the XOR of base and the rows c_2 .. c_p that a lane keeps in registers
// ranks per workgroup: as many as kSumsMaxRanks, so that the first unranking and the copy of S are shared by many outputs, halved
// down to kSumsMinRanks while there are fewer than kSumsWantGroups workgroups
constexpr int kSumsMinRanks = 1024;
constexpr int kSumsMaxRanks = 16384;
constexpr int kSumsWantGroups = 2048;

struct SumsPlan {
  int id;            // the kernel: 0 .. 3 S in LDS with 1, 2, 8, 64 lanes per row; 4 .. 7 S from global memory likewise; -1: bad shape
  int lanes;         // lanes per row
  int staged;        // S in LDS
  long long ranks;   // ranks per workgroup R
  long long lds;     // LDS bytes per workgroup
  long long groups;  // workgroups
};

inline SumsPlan sums_plan(long long n, long long ncols, int p, long long count) {
  const SumsPlan bad = {-1, 0, 0, 0, 0, 0};
  const long long total = sums_count(n, p);
  if (n < 0 || ncols < 0 || count < 0 || total < 0 || count > total || n > 0x7FFFFFFFll || ncols > 0x7FFFFFFFll) return bad;
  SumsPlan s;
  const long long nw = (ncols + 63) >> 6;
  s.lanes = nw <= kLf2PieceWords ? 1 : nw <= kLf2NarrowWords ? 2 : nw <= kLf2MidWords ? 8 : 64;
  const long long image = 8 * (n + 1) * (nw ? nw : 1);
  s.staged = image <= kSumsLdsBytes;
  s.lds = s.staged ? lf2_align16(image) : 0;
  s.id = (s.staged ? 0 : 4) + (s.lanes == 1 ? 0 : s.lanes == 2 ? 1 : s.lanes == 8 ? 2 : 3);
  s.ranks = kSumsMaxRanks;
  while (s.ranks > kSumsMinRanks && count / s.ranks < kSumsWantGroups) s.ranks >>= 1;
  s.groups = (count + s.ranks - 1) / s.ranks;
  return s;
}
