// gf2_join.h -- launchers of gf2_join.hip (callers: join_host.cpp).  Arguments are checked by the callers.  Every launcher only
// enqueues on `stream`.  skeys_a / skeys_b: the sorted keys of A and B (gf2k_lf2_sort_pass), order_a / order_b: their rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// sums[k] = the outputs of the runs of A before run k (join_plan: `runs` runs of kJoinRunRows sorted positions), *count = the outputs
// of all.  nrows_a > 0, nrows_b > 0
hipError_t gf2k_join_count(const int *skeys_a, int nrows_a, const int *skeys_b, int nrows_b, long long *sums, long long *count,
                           hipStream_t stream);
// D[offsets[run] + j] = A[order_a[s]] ^ B[order_b[p]] for the outputs below cap; ia / ib / wt (each may be null) get order_a[s],
// order_b[p] and the ones of D's row in the columns [wc0, wc1).  nrows_a > 0, nrows_b > 0, cap > 0.  lanes: -1, what join_plan says;
// 1, 2, 8 or 64: that kernel, for the benchmark
hipError_t gf2k_join_scatter(const uint64_t *A, long long lda, int nrows_a, const uint64_t *B, long long ldb, int nrows_b, int ncols,
                             const int *order_a, const int *skeys_a, const int *order_b, const int *skeys_b, const long long *offsets,
                             uint64_t *D, long long ldd, int cap, int *ia, int *ib, int *wt, int wc0, int wc1, int lanes,
                             hipStream_t stream);

// ---- the weight-filtered join (gf2_join_select.inc)
// hown[k] = the hits of run k of A: its pairs whose XOR has between wlo and whi ones in the columns [wc0, wc1); hsums[k] = the hits of
// the runs before k, *hits = the hits of all.  nrows_a > 0, nrows_b > 0.  lanes: -1, what join_select_plan says by the words of the
// range; 1, 2, 8 or 64: that kernel, for the benchmark
hipError_t gf2k_join_weigh(const uint64_t *A, long long lda, int nrows_a, const uint64_t *B, long long ldb, int nrows_b, int ncols,
                           const int *order_a, const int *skeys_a, const int *order_b, const int *skeys_b, long long *hsums, long long *hown,
                           long long *hits, int wc0, int wc1, int wlo, int whi, int lanes, hipStream_t stream);
// D[hoffs[run] + h] = A[order_a[s]] ^ B[order_b[p]] for hit h of the run, in the order of its outputs, for the hits below cap; ia / ib /
// wt (each may be null) beside it.  D null: the rows are not stored.  nrows_a > 0, nrows_b > 0, cap > 0.  lanes: -1, what join_plan says
// by the row width; 1, 2, 8 or 64: that kernel
hipError_t gf2k_join_select_scatter(const uint64_t *A, long long lda, int nrows_a, const uint64_t *B, long long ldb, int nrows_b, int ncols,
                                    const int *order_a, const int *skeys_a, const int *order_b, const int *skeys_b, const long long *hoffs,
                                    const long long *hown, uint64_t *D, long long ldd, int cap, int *ia, int *ib, int *wt, int wc0, int wc1,
                                    int wlo, int whi, int lanes, hipStream_t stream);
}
