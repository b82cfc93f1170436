// gf2_unique.h -- launchers of gf2_unique.hip (callers: unique_host.cpp).  Arguments are checked by the callers.  Every launcher only
// enqueues on `stream`.  value(i) = the bits [c0, c1) of row i of P; nrows > 0 throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// pairs[i] = (the bits [wc0, wc0 + bits) of row r of P, r), r = i if `first`, else the row that pairs[i] holds: one window's keys in
// the order the windows below it have left.  In place: `pairs` is nrows pairs of int32 (key, row).  1 <= bits <= kUniqueWindowBits
hipError_t gf2k_unique_rekey(const uint64_t *P, long long ld, int wc0, int bits, int nrows, int first, void *pairs, hipStream_t stream);
// head[s] = the first sorted position of the class of position s, for the sorted `order` of P's rows.  carry: unique_plan: `runs`
// int32 of work space, written before they are read
hipError_t gf2k_unique_heads(const uint64_t *P, long long ld, int nrows, int c0, int c1, const int *order, int *head, int *carry,
                             hipStream_t stream);
// rep[order[s]] = order[head[s]] (rep may be null) and flags[i] = (rep[i] == i), nrows int32 each
hipError_t gf2k_unique_rep(const int *order, const int *head, int nrows, int *rep, int *flags, hipStream_t stream);
}
