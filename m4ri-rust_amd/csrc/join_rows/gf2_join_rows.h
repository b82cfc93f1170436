// gf2_join_rows.h -- the launchers of gf2_join_rows.hip (caller: join_rows_host.cpp).  Arguments are checked by the caller.  Everything
// here only enqueues on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// pairs[i] = (bits [shift, shift + bits) of rep[row], row), an int32 pair as the passes of the class sort take them: row = i where
// `first`, else the row that pairs[i] holds (the order a window below has left).  nrows > 0, 1 <= bits <= 30
hipError_t gf2k_join_rows_pairs(const int *rep, int nrows, int shift, int bits, int first, void *pairs, hipStream_t stream);
// start[r] = s for every sorted position s whose row r = order[s] is the lowest of its class (rep[r] == r); no other word of start
// is written.  nrows > 0
hipError_t gf2k_join_rows_starts(const int *order, const int *rep, int nrows, int *start, hipStream_t stream);
// head[s] = start[rep[order[s]]]: the first sorted position of the class of position s.  nrows > 0
hipError_t gf2k_join_rows_heads(const int *order, const int *rep, const int *start, int nrows, int *head, hipStream_t stream);
// sums[k] = the sum of mult over the runs before run k of A (join_rows_plan: `runs` runs of kJoinRowsRunRows rows), *count = the sum
// of all: two launches.  nrows_a > 0
hipError_t gf2k_join_rows_count(const int *mult, int nrows_a, long long *sums, long long *count, hipStream_t stream);
// offs[i] = the sum of mult over the rows before row i, from the run offsets that gf2k_join_rows_count left in sums.  nrows_a > 0
hipError_t gf2k_join_rows_offsets(const int *mult, int nrows_a, const long long *sums, long long *offs, hipStream_t stream);
// for t < min(*count, cap): output t belongs to row i of A, the largest with offs[i] <= t, and to row j = order_b[start[idx[i]] + t -
// offs[i]] of B: D[t] = A[i] ^ B[j] (D null: not stored), ia[t] = i, ib[t] = j, wt[t] = the ones of A[i] ^ B[j] in [wc0, wc1) (each may
// be null).  The grid runs over the chunks of `cap` outputs.  nrows_a > 0, cap > 0.  lanes: -1, what join_rows_plan says; 1, 2, 8 or
// 64: that kernel, for the benchmark
hipError_t gf2k_join_rows_scatter(const uint64_t *A, long long lda, int nrows_a, const uint64_t *B, long long ldb, int nrows_b, int ncols,
                                  const int *idx, const long long *offs, const int *order_b, const int *start, const long long *count,
                                  uint64_t *D, long long ldd, int cap, int *ia, int *ib, int *wt, int wc0, int wc1, int lanes,
                                  hipStream_t stream);
}
