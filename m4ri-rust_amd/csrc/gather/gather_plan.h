// gather_plan.h -- which path a column gather takes, in ONE place: gf2_gather_cols_dev launches what this says and gf2_gather_cols_plan
// reports it (the way mul_plan.h serves the products).  Plain host arithmetic, no HIP.
#pragma once

// the fused kernel (gf2_gather.hip: gf2_gather_cols_kernel)
constexpr int kGatherBandRows = 64;      // rows a workgroup owns: one bit of an LDS word each
constexpr int kGatherThreads = 1024;     // sixteen waves: one 64 x 64 block each per step, 16 lanes on the 16 staged words of a row
constexpr int kGatherStageWords = 16;    // word columns of D staged per step
// The LDS image is 8 bytes per source column (rounded up to whole words of S) plus two staging buffers of 64 rows x 16 words for the
// way out.  The fused kernel is planned for HALF the 160 KiB of a CU, so that two workgroups are resident and one stages its band
// while the other gathers: 8192 source columns at the most.
constexpr long long kGatherLdsBudget = 80 * 1024;
constexpr long long kGatherStageBytes = 2 * 8ll * kGatherBandRows * kGatherStageWords;

struct GatherColsPlan {
  int path;             // 0: fused LDS kernel, 1: transpose -> row gather -> transpose, -1: bad shape
  long long threads;    // per workgroup of the fused kernel (path 1: of the row gather)
  long long lds_bytes;  // per workgroup (path 1: 0)
  long long rows;       // per workgroup (path 1: 0)
  long long scratch;    // bytes of stream scratch (path 0: 0)
};

inline long long gather_ld_for(long long ncols) {  // the even row stride of a scratch matrix
  const long long w = (ncols + 63) >> 6;
  return w <= 1 ? 1 : ((w + 1) & ~1ll);
}

inline GatherColsPlan gather_cols_plan(long long nrows, long long s_ncols, long long d_ncols) {
  if (nrows < 0 || s_ncols < 0 || d_ncols < 0) return {-1, 0, 0, 0, 0};
  const long long lds = 8 * 64 * ((s_ncols + 63) >> 6) + kGatherStageBytes;
  if (lds <= kGatherLdsBudget) return {0, kGatherThreads, lds, kGatherBandRows, 0};
  // S^T (s_ncols x nrows) in one slot, the gathered rows (d_ncols x nrows) in another
  const long long ldt = gather_ld_for(nrows);
  return {1, 256, 0, 0, 8 * ldt * (s_ncols + d_ncols)};
}
