// gf2_near.h -- launchers of gf2_near.hip (callers: near_host.cpp).  Arguments are checked by the callers.  Every launcher only
// enqueues on `stream`.  cells: the scratch of near_plan, one int64 per (row of A, chunk of B) in the order of near_cell, and one more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the two pools, the range and the flags of a call.  nrows_a > 0, nrows_b > 0
struct NearOperands {
  const uint64_t *A;
  long long lda;
  int nrows_a;
  const uint64_t *B;
  long long ldb;
  int nrows_b;
  int ncols, wc0, wc1, flags;
};

extern "C" {
// cells[cell] = the hits before that cell, cells[NA * S] = *hits = the hits of all: the admitted pairs with wlo <= d <= whi
hipError_t gf2k_near_count(const NearOperands *o, int wlo, int whi, long long *cells, long long *hits, hipStream_t stream);
// the hits of every cell, in ascending row of B, from cells[cell] on: D (null: the rows are not stored), ia / ib / wt (each may be
// null), for the hits below cap.  cells: as gf2k_near_count left them.  cap > 0
hipError_t gf2k_near_select(const NearOperands *o, int wlo, int whi, const long long *cells, uint64_t *D, long long ldd, int cap, int *ia,
                            int *ib, int *wt, hipStream_t stream);
// idx[i] / dist[i] (either may be null) = the lowest nearest admitted row of B and its distance, -1 where there is none; the minima
// of the chunks go through cells
hipError_t gf2k_nearest(const NearOperands *o, long long *cells, int *idx, int *dist, hipStream_t stream);
}
