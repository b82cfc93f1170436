// gf2_weight.h -- launchers of gf2_weight.hip (callers: weight_host.cpp; gf2k_weight_select also unique/unique_host.cpp).  Arguments are checked by the callers; an empty A launches
// nothing (the callers clear the output).  Every launcher only enqueues on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// weights[i] = set bits of row i; the kernel weight_rows_plan() names.  gf2k_weight_rows_narrow is the launcher of its variant 0
hipError_t gf2k_weight_rows(const uint64_t *A, long long ld, int nrows, int ncols, int *weights, hipStream_t stream);
hipError_t gf2k_weight_rows_narrow(const uint64_t *A, long long ld, int nrows, int ncols, int *weights, hipStream_t stream);
// *total += set bits of A: the caller has cleared *total on `stream`
hipError_t gf2k_weight_total(const uint64_t *A, long long ld, int nrows, int ncols, unsigned long long *total, hipStream_t stream);
// weights[j] = rows with bit j set.  partial: weight_cols_plan().scratch bytes when the plan has more than one band (else unused)
hipError_t gf2k_weight_cols(const uint64_t *A, long long ld, int nrows, int ncols, int *weights, int *partial, hipStream_t stream);
// idx[0 .. min(*count, cap)) = the i < n with lo <= weights[i] <= hi, ascending; *count = how many.  block_counts: scratch of
// ceil(n / kWeightSelectBlock) ints.  n > 0
hipError_t gf2k_weight_select(const int *weights, int n, int lo, int hi, int *idx, int cap, int *count, int *block_counts,
                              hipStream_t stream);
}
