// gf2_cover.h -- launcher of gf2_cover.hip (caller: cover_host.cpp).  Arguments are checked by the caller.  It only enqueues on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/m4ri_hip_cover.h"

extern "C" {
// D[i] = the messages of the blocks of row i of P from column c0 on, dist[i] (may be null) the weight of what was removed.  nrows > 0.
// codes, seg_code (host) and the window are legal (cover_plan.h); tables: host array of ncodes device pointers, one for every code
// with a table that a segment uses.  variant: -1, what cover_plan says; 0 or 1 (1 only where the plan's span is at most
// kCoverStageWords): that kernel, for the benchmark
hipError_t gf2k_cover_reduce(const uint64_t *P, long long ld, int nrows, int p_ncols, int c0, const gf2_cover_code *codes, int ncodes,
                             const unsigned char *seg_code, int nseg, const uint32_t *const *tables, uint64_t *D, long long ldd, int *dist,
                             int variant, hipStream_t stream);
}
