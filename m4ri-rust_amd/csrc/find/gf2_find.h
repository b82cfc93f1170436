// gf2_find.h -- the launcher of gf2_find.hip (caller: find_host.cpp).  Arguments are checked by the caller.  It only enqueues on
// `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// idx[i] = the lowest row of B that equals row i of A on the columns [c0, c1), -1 for none; mult[i] (may be null) = the number of such
// rows; *count (may be null) = the rows of A with idx[i] >= 0.  table: find_plan(...).scratch bytes of work space, filled by the first
// of the three launches.  nrows_a > 0 and nrows_b > 0
hipError_t gf2k_find_rows(const uint64_t *A, long long lda, int nrows_a, const uint64_t *B, long long ldb, int nrows_b, int c0, int c1,
                          void *table, int *idx, int *mult, int *count, hipStream_t stream);
}
