// gf2_bkw.h -- launchers of gf2_bkw.hip (callers: bkw_host.cpp).  Arguments are checked by the callers.  Every launcher only enqueues
// on `stream`.  key(i) = bits [c0, c0 + b) of row i of P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// first[v] = min(first[v], the lowest row with key v) as unsigned values.  The caller has set the 2^b entries to all-ones bytes on
// `stream`.  nrows > 0: nothing is launched otherwise.  variant: -1, what lf1_first_variant(b) says; 0 (b <= kLf1LdsLevels) or 1: that
// kernel, for the benchmark
hipError_t gf2k_lf1_first(const uint64_t *P, long long ld, int nrows, int c0, int b, int *first, int variant, hipStream_t stream);
// block_counts[k] = the survivors among the rows of block k (lf1_plan: `rows` rows each); first is finished.  nrows > 0
hipError_t gf2k_lf1_count(const uint64_t *P, long long ld, int nrows, int ncols, int c0, int b, int keep_zero, const int *first,
                          int *block_counts, hipStream_t stream);
// block_counts[k] becomes the sum of the counts before k, *count the sum of all
hipError_t gf2k_lf1_scan(int *block_counts, long long nblk, int *count, hipStream_t stream);
// D[offsets[block] + rank] = survivor ^ its class first, for positions below cap; src (may be null) gets the survivors' rows.
// nrows > 0, cap > 0.  lanes: -1, what lf1_plan says; for the benchmark, rows of up to kLf1NarrowWords words also take 1 or 2
hipError_t gf2k_lf1_scatter(const uint64_t *P, long long ld, int nrows, int ncols, int c0, int b, int keep_zero, const int *first,
                            const int *offsets, uint64_t *D, long long ldd, int cap, int *src, int lanes, hipStream_t stream);
}
