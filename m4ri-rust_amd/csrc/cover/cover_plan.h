// cover_plan.h -- the rules of a covering-code reduction, in ONE place: what a legal code is, how the segments lie in the rows, and how
// the kernel runs.  cover_host.cpp checks and reports with these, the launcher of gf2_cover.hip launches what cover_plan says (the way
// bkw_plan.h serves an LF1 round).  Plain host arithmetic, no HIP.
#pragma once
#include <stdint.h>

#include "../../../include/m4ri_hip_cover.h"

constexpr int kCoverThreads = 256;   // a workgroup; it covers kCoverThreads rows per pass, a lane per row in the decode
// The window of a row can touch at most `span` words.  Up to kCoverStageWords the workgroup first copies the window words of its rows
// into LDS, `lanes` lanes per row and a word per lane, so that a wave reads consecutive words; every lane then decodes its own row from
// LDS.  Above, a lane reads the words of its row from global memory as the blocks need them (DESIGN.md section 7.12 has both measured
// where both are possible).
constexpr int kCoverStageWords = 8;
constexpr int kCoverMaxGroups = 2048;   // workgroups at the most: they loop over the passes, so the tables are copied once each

// 0: the code is legal (include/m4ri_hip_cover.h); else which rule it breaks: 1 n, 2 k, 3 r, 4 a bit of h at or above n, 5 h is not
// systematic.  h is read only for 1 <= k < n.
inline int cover_code_fault(const gf2_cover_code &c) {
  if (c.n < 1 || c.n > GF2_COVER_MAX_N) return 1;
  if (c.k < 0 || c.k > c.n) return 2;
  if (c.k == 0 || c.k == c.n) return 0;
  const int r = c.n - c.k;
  if (r > GF2_COVER_MAX_R) return 3;
  for (int t = 0; t < r; ++t) {
    if (c.n < 32 && (c.h[t] >> c.n)) return 4;
    if ((c.h[t] >> c.k) != (1u << t)) return 5;
  }
  return 0;
}
inline const char *cover_fault_text(int fault) {
  static const char *const text[] = {"", "n is outside 1 <= n <= 32", "k is outside 0 <= k <= n", "r = n - k is above 12",
                                     "h has a bit at or above n", "h is not systematic (h[t] >> k must be 1 << t)"};
  return text[fault];
}
inline bool cover_has_table(const gf2_cover_code &c) { return c.k > 0 && c.k < c.n; }

struct CoverPlan {
  int variant;        // 0: rows read from global memory, 1: window words staged in LDS; -1: a bad argument
  int lanes;          // lanes per row of the copy into LDS (1 for variant 0)
  int span;           // the words of a row that the window can touch, at the most
  long long lds;      // bytes: the tables, then the staged words
  long long K, bits;  // columns of D, bits of the window
  long long table_words;
  long long blocks;
};

// codes / seg_code may be null where their count is 0
inline CoverPlan cover_plan(long long nrows, long long p_ncols, const gf2_cover_code *codes, int ncodes, const unsigned char *seg_code,
                            int nseg) {
  const CoverPlan bad = {-1, 0, 0, 0, 0, 0, 0, 0};
  if (nrows < 0 || p_ncols < 0 || nseg < 0 || nseg > GF2_COVER_MAX_SEGS || ncodes < 0 || ncodes > GF2_COVER_MAX_CODES) return bad;
  if (ncodes == 0 && nseg > 0) return bad;
  if ((ncodes > 0 && !codes) || (nseg > 0 && !seg_code)) return bad;
  CoverPlan p = {0, 1, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < ncodes; ++c) {
    if (cover_code_fault(codes[c])) return bad;
    if (cover_has_table(codes[c])) p.table_words += 1ll << (codes[c].n - codes[c].k);
  }
  if (p.table_words > GF2_COVER_MAX_LEADERS) return bad;
  for (int j = 0; j < nseg; ++j) {
    if (seg_code[j] >= ncodes) return bad;
    p.K += codes[seg_code[j]].k;
    p.bits += codes[seg_code[j]].n;
  }
  if (p.bits > p_ncols) return bad;
  const long long nw = (p_ncols + 63) >> 6, reach = p.bits ? ((p.bits + 62) >> 6) + 1 : 0;   // at the worst bit offset
  p.span = (int)(reach < nw ? reach : nw);
  if (p.span > 0 && p.span <= kCoverStageWords) {
    p.variant = 1;
    while (p.lanes < p.span) p.lanes *= 2;
  }
  p.lds = 4 * p.table_words + (p.variant == 1 ? 8ll * kCoverThreads * (p.span | 1) : 0);
  const long long passes = (nrows + kCoverThreads - 1) / kCoverThreads;
  p.blocks = passes < kCoverMaxGroups ? passes : kCoverMaxGroups;
  return p;
}
