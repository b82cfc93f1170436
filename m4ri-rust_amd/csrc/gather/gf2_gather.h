// gf2_gather.h -- launchers of gf2_gather.hip (callers: gather_host.cpp).  Arguments are checked by the callers; shapes may be empty.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// D[i] (^)= S[idx[i]], i < d_nrows, rows of ncols bits; idx and bad are device pointers (bad may be null)
hipError_t gf2k_gather_rows(uint64_t *D, long long ldd, const uint64_t *S, long long lds_, int d_nrows, int s_nrows, int ncols,
                            const int *idx, int accumulate, int *bad, hipStream_t stream);
// D[r][j] = S[r][idx[j]], r < nrows, j < d_ncols: the fused kernel; hipErrorInvalidValue when gather_cols_plan() does not name it
hipError_t gf2k_gather_cols(uint64_t *D, long long ldd, int d_ncols, const uint64_t *S, long long lds_, int s_ncols, int nrows,
                            const int *idx, int *bad, hipStream_t stream);
}
