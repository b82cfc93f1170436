// gf2_draw.h -- launchers of gf2_draw.hip (callers: draw_host.cpp).  Arguments are checked by the callers.  Every launcher only
// enqueues on `stream`.  The values are those of philox.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// word (r, j) of D (^)= the noise word (row0 + r) * fullw + colw0 + j, the last word of a row masked.  rows > 0, cols > 0, thr > 0
hipError_t gf2k_bernoulli(uint64_t *D, long long ld, int rows, int cols, uint32_t thr, uint64_t seed, long long row0, long long fullw,
                          long long colw0, int accumulate, hipStream_t stream);
// idx[t] = the draw t below n, t < count.  count > 0
hipError_t gf2k_draw_indices(int *idx, long long count, uint32_t n, uint64_t seed, hipStream_t stream);
// sub[g * k + t]: `batch` ordered k-tuples of distinct values below n, -1 where a position has not settled after max_rounds rounds;
// *unfinished (may be null, zeroed by the caller on the stream) += the subsets with such a position.  batch > 0
hipError_t gf2k_draw_subsets(int *sub, int batch, int k, uint32_t n, uint64_t seed, int max_rounds, int *unfinished, hipStream_t stream);
// pairs[i] = (key(i), i), i < n: n pairs of int32, the input of pass 0 of the class sort.  n > 0
hipError_t gf2k_draw_perm_pairs(void *pairs, int n, uint64_t seed, hipStream_t stream);
}
