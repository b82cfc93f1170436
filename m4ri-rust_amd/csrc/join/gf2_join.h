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
}
