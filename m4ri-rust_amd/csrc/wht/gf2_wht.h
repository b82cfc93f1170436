// gf2_wht.h -- launchers of gf2_wht.hip (callers: wht_host.cpp).  Arguments are checked by the callers.  Every launcher only enqueues
// on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// f[v] += (rows of P whose bits [c0, c0 + k) read v and whose bit label_col is 0) - (... is 1); label_col < 0: every row counts + 1.
// The caller has cleared f on `stream`.  nrows > 0
hipError_t gf2k_wht_tally(const uint64_t *P, long long ld, int nrows, int c0, int k, int label_col, unsigned *f, hipStream_t stream);
// the passes of wht_plan(k) over f (2^k values, 16-byte aligned when k >= 2).  fold: the last pass stores (n - F) / 2 instead of F.
// k == 0 launches nothing unless fold
hipError_t gf2k_wht_transform(unsigned *f, int k, int fold, unsigned n, hipStream_t stream);
// one pass of that plan alone (for the benchmark): pass p of wht_plan(k)
hipError_t gf2k_wht_pass(unsigned *f, int k, int p, int fold, unsigned n, hipStream_t stream);
// *val = min of w[0 .. n), *idx = the lowest index that holds it.  partial: wht_min_scratch(n) bytes.  n >= 1
hipError_t gf2k_wht_min(const int *w, int n, int *idx, int *val, int *partial, hipStream_t stream);
}
