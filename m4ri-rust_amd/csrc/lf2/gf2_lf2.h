// gf2_lf2.h -- launchers of gf2_lf2.hip and the enqueue of the whole class sort (lf2_host.cpp; callers: lf2_host.cpp, join_host.cpp,
// draw_host.cpp, unique_host.cpp).  Arguments are checked by the callers.  Everything here only enqueues on `stream`.  key(i) = bits [c0, c0 + b) of row i of P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/m4ri_hip.h"

extern "C" {
// One pass of the sort, 0 <= pass < lf2_plan(...).passes, over the key bits [8 * pass, ...): stable.  P non-null (the first pass): the
// items are (key(i), i); else `in`, nrows pairs of int32 (key, row).  order non-null (the last pass): order[place] = row and, skeys
// non-null, skeys[place] = key; else `out` receives the pairs.  counts (256 * tiles int32 at the most) and parts (lf2_plan: part_bytes)
// are work space, written before they are read.  nrows > 0
hipError_t gf2k_lf2_sort_pass(const uint64_t *P, long long ld, int c0, int b, const void *in, int nrows, int pass, int *counts, int *parts,
                              void *out, int *order, int *skeys, hipStream_t stream);
// order[i] = i and (skeys non-null) skeys[i] = 0: the sort for b == 0
hipError_t gf2k_lf2_iota(int nrows, int *order, int *skeys, hipStream_t stream);
// sums[k] = the outputs of the runs before run k (lf2_plan: `runs` runs of kLf2RunRows sorted positions), *count = the outputs of all.
// nrows > 0
hipError_t gf2k_lf2_pair_count(const int *skeys, int nrows, long long *sums, long long *count, hipStream_t stream);
// D[offsets[run] + j] = P[order[s]] ^ P[order[p]] for the outputs below cap; lo / hi (each may be null) get order[p] / order[s].
// nrows > 0, cap > 0.  lanes: -1, what lf2_plan says; 1, 2, 8 or 64: that kernel, for the benchmark
hipError_t gf2k_lf2_pair_scatter(const uint64_t *P, long long ld, int nrows, int ncols, const int *order, const int *skeys,
                                 const long long *offsets, uint64_t *D, long long ldd, int cap, int *lo, int *hi, int lanes,
                                 hipStream_t stream);
}

// order and (unless null) skeys <- the stable sort of M's rows by their key: the iota for b == 0, else the passes in turn, the first on
// the matrix, the last into order.  work: lf2_plan(M->nrows, M->ncols, b).sort_scratch bytes (lf2_sort_work cuts them; unused for
// b == 0), the caller's.  M->nrows > 0; the caller holds gf2_enqueue_mu.  fn: the entry's name, for the message of a failed launch
int gf2_enqueue_class_sort(const char *fn, gf2_dmat const *M, int c0, int b, void *work, int *order, int *skeys, hipStream_t stream);
