// gf2_sums.h -- launchers of gf2_sums.hip (callers: sums_host.cpp).  Arguments are checked by the callers.  Every launcher only enqueues
// on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// D[t] = base ^ S[c_1] ^ ... ^ S[c_p] for the subset of rank rank0 + t, t < count; idx[t * p + i - 1] = c_i; wt[t] = the ones of D[t] in
// the columns [wc0, wc1).  base, D, idx and wt may each be null (D: rows not stored), but not D, idx and wt all three.  n >= p, count
// > 0, 0 <= rank0, rank0 + count <= C(n, p).  global_s: 0, the kernel that sums_plan says; 1: S is read from global memory also
// where it would fit LDS, for the benchmark
hipError_t gf2k_subset_sums(const uint64_t *S, long long lds, int n, const uint64_t *base, int ncols, int p, long long rank0, long long count,
                            uint64_t *D, long long ldd, int *idx, int *wt, int wc0, int wc1, int global_s, hipStream_t stream);
// idx[t * p ..] = the subset of rank rank0 + ranks[t], t < count; p times -1 for ranks[t] == -1 and for a rank outside [0, C(n, p)),
// which also stores 1 to *bad (bad may be null).  count > 0, 1 <= p <= 4, C(n, p) <= 2^62
hipError_t gf2k_unrank_subsets(const int *ranks, int count, long long rank0, int p, int n, int *idx, int *bad, hipStream_t stream);
}
