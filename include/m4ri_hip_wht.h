/* m4ri_hip_wht.h -- companion of m4ri_hip.h, section 2 (device-resident API): the exhaustive LPN solve ON THE DEVICE.  After a
 * reduction (BKW / LF1, covering codes) a solver is left with N samples of k bits, k about 16 to 30, and must score all 2^k secrets:
 * tally the samples into f[v] = #(sample = v, label 0) - #(sample = v, label 1), apply one fast Walsh-Hadamard transform
 * F[s] = sum over v of (-1)^<s,v> f[v], and read errors[s] = (N - F[s]) / 2 -- N + k 2^k additions instead of N k 2^k bit operations.
 * errors[s] has exactly the meaning of gf2_col_weights_dev(pool * [S ; 1]) for S = all 2^k vectors (m4ri_hip_weight.h), so
 * gf2_select_weights_dev and the gathers take it as it is; gf2_min_weight_dev names the best secret.  DESIGN.md section 7.10;
 * INTEGRATION.md sections 3 and 4.
 *
 * Outputs are OVERWRITTEN: the caller zeroes nothing.  The results are exact integers and do not depend on launch order or on how
 * workgroups interleave: only integer adds, in unsigned arithmetic, so wrap-around is defined.  gf2_wht_dev is arithmetic modulo 2^32
 * (exact whenever the true value fits); in gf2_lpn_errors_dev the sum of |f| is nrows < 2^31, so F and errors never wrap.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  gf2_lpn_errors_dev works inside `errors`
 * (no other scratch).  gf2_min_weight_dev takes scratch from the stream's arena (gf2_wht_plan, out[11]); every partial that is read
 * has been written by the same call.  Ties go to the LOWEST index, so two runs give the same answer.
 *
 * The index.  Bit j of v is column c0 + j of P.  c0 may be any bit offset: because k <= 30 the index spans at most two words of a
 * row.  label_col may be any column of P, one inside the index range included; label_col == -1 (gf2_lpn_tally_dev only) means no
 * label: f is the plain histogram.
 *
 * What is read.  Only the words of a row that hold the index bits and the label bit: excess bits and the words between the row width
 * and `ld` are never read, so P may be a strided view of a dirty parent.  Rows that are only 8-byte aligned (an odd `ld`, a base on an
 * odd word) are accepted, and rows are addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of P is written.
 *
 * Empty and degenerate shapes.  nrows == 0: the tally gives zeros, and so does gf2_lpn_errors_dev.  k == 0: an array of one element
 * (f[0] = rows with label 0 - rows with label 1); the transform is the identity and needs no device.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null P, a null `data` on a non-empty P, a null
 * output, a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, an array that is not 4-byte aligned,
 * a k outside 0 <= k <= 30, a column range [c0, c0 + k) or a label column outside P (gf2_lpn_errors_dev: label_col == -1 too) and
 * n < 1 return -1 and set gf2_last_error to a text that starts with the entry's name.  The transform moves 16 bytes per access: the
 * array of gf2_wht_dev and of gf2_lpn_errors_dev must be 16-byte aligned when k >= 2 (what hipMalloc returns is), else -1.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  The address range of an output may not meet P's address range.  For
 * gf2_min_weight_dev, `idx` and `val` may meet neither `w` (n ints) nor each other. */
#ifndef M4RI_HIP_WHT_H
#define M4RI_HIP_WHT_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* f[v] = (# rows i of P whose bits [c0, c0+k) read v and whose bit label_col is 0) - (# ... is 1),   v in [0, 2^k);
 * bit j of v is column c0 + j.  label_col == -1: no label, f is the plain histogram.  f: DEVICE int32[2^k], OVERWRITTEN. */
int gf2_lpn_tally_dev(gf2_dmat const *P, int c0, int k, int label_col, int *f, void *stream);
/* in place: f[s] <- sum over v of (-1)^popcount(s & v) * f[v], 2^k int32, arithmetic modulo 2^32 (exact whenever the true value fits) */
int gf2_wht_dev(int *f, int k, void *stream);
/* errors[s] = # rows i with <P[i][c0 .. c0+k), s> != P[i][label_col], for EVERY s in [0, 2^k): tally, transform, (N - F) / 2,
 * all inside `errors` (DEVICE int32[2^k], OVERWRITTEN; no other scratch).  label_col is required here (>= 0). */
int gf2_lpn_errors_dev(gf2_dmat const *P, int c0, int k, int label_col, int *errors, void *stream);
/* *val = the smallest of w[0 .. n), *idx = the LOWEST index that holds it; w, idx, val DEVICE; n >= 1 */
int gf2_min_weight_dev(const int *w, int n, int *idx, int *val, void *stream);
/* without a device: how a transform of 2^k runs.  Returns the number of passes over the array (0 for k == 0), -1 for a bad k;
 * out[0 .. 7] = first level of pass p (pass p covers levels [out[p], out[p+1]), unused entries = k), out[8] = threads per
 * workgroup, out[9] = LDS bytes (of a workgroup of the first pass; the later passes take none), out[10] = tally variant (0:
 * per-workgroup histogram in LDS, 1: atomics straight into f), out[11] = scratch bytes of gf2_min_weight_dev for n = 2^k.  out may
 * be NULL. */
int gf2_wht_plan(int k, long long out[12]);

#ifdef __cplusplus
}
#endif
#endif
