/* m4ri_hip_weight.h -- companion of m4ri_hip.h, section 2 (device-resident API): Hamming weights of a device matrix -- of its rows, of
 * its columns, of the whole matrix -- and the indices whose weight lies in a window, all ON THE DEVICE.  The verdict of an LPN solver
 * (the weight of column b of pool * [S ; 1] is the number of samples that candidate b gets wrong) and of information-set decoding (a
 * row of weight <= w after the elimination) stay on the caller's stream with these, and the selected indices feed
 * gf2_gather_rows_dev / gf2_gather_cols_dev (m4ri_hip_gather.h) as they are.  DESIGN.md section 7.9; INTEGRATION.md sections 3 and 4.
 *
 * Outputs are OVERWRITTEN: the caller zeroes nothing (unlike `bad` of the gathers).  Entries of `idx` from min(*count, cap) on are not
 * touched.  The results are exact integers and do not depend on launch order or on how workgroups interleave.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  Column weights of a matrix with more than one
 * band of rows (gf2_weights_plan, out[3]) and gf2_select_weights_dev take scratch from the stream's arena; every scratch word that a
 * kernel reads has been written by the same call.
 *
 * What counts.  Only the `ncols` bits of each row: the excess bits of the last word never reach a result, and words between the row
 * width and `ld` are never read, so A may be a strided view of a dirty parent.  Rows that are only 8-byte aligned (an odd `ld`, a base
 * on an odd word) are accepted; 16-byte loads are used only where every row starts on a 16-byte boundary.  Nothing of A is written.
 *
 * Empty shapes.  An output of length 0 returns 0 without a device: nrows == 0 for rows, ncols == 0 for columns, n == 0 with cap == 0
 * for select (`count` is then not written).  Otherwise an empty A gives zeros: the row weights of an m x 0 matrix, the column weights
 * of a 0 x n matrix, *total = 0.  lo > hi selects nothing: *count = 0.  cap == 0 with idx == NULL is a count-only call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null A, a null `data` on a non-empty matrix, a
 * null output where its length is non-zero, a null `count`, a null `idx` with cap > 0, a negative dimension, n or cap, an `ld` below
 * the row width, a `data` that is not 8-byte aligned, a `weights` or `idx` that is not 4-byte aligned and a `total` that is not 8-byte
 * aligned return -1 and set gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  The address range of an output may not meet A's address range.  For
 * select, `idx` (cap ints) and `count` may meet neither `weights` (n ints) nor each other.
 *
 * Sizes.  Dimensions are below 2^31, so every weight fits an int32; rows are addressed with 64-bit offsets, so operands past 4 GiB
 * work; the total is a 64-bit count (nrows * ncols can pass 2^32). */
#ifndef M4RI_HIP_WEIGHT_H
#define M4RI_HIP_WEIGHT_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* weights[i] = number of set bits in row i of A.       weights: DEVICE int32[A->nrows] */
int gf2_row_weights_dev(gf2_dmat const *A, int *weights, void *stream);
/* weights[j] = number of rows of A with bit j set.     weights: DEVICE int32[A->ncols] */
int gf2_col_weights_dev(gf2_dmat const *A, int *weights, void *stream);
/* *total = number of set bits of A.                     total: DEVICE uint64 (nrows * ncols can pass 2^32) */
int gf2_count_ones_dev(gf2_dmat const *A, unsigned long long *total, void *stream);
/* idx[0 .. min(*count, cap)) = the i < n with lo <= weights[i] <= hi, ASCENDING; *count = how many there are in all (may exceed cap).
 * weights, idx, count: DEVICE.  idx feeds gf2_gather_rows_dev / gf2_gather_cols_dev as it is. */
int gf2_select_weights_dev(const int *weights, int n, int lo, int hi, int *idx, int cap, int *count, void *stream);
/* which kernel a shape runs on, without a device (what: 0 rows, 1 columns, 2 total); returns a variant id, -1 for a bad shape (a
 * negative dimension, another `what`);
 *   rows:    0 = one lane per row (rows of up to 4 words), 1 = 8 or 64 lanes per row;
 *   columns: 0 = one band of rows, stored straight into `weights`, 1 = several bands, per-band sums in scratch and a fold launch;
 *   total:   0, 1, 2 = 1, 8, 64 lanes per row.
 * out[0] = threads per workgroup, out[1] = rows per workgroup (per pass of the row loop), out[2] = rows a lane takes before it
 * empties its bit-sliced counters (columns; 0 otherwise), out[3] = scratch bytes.  Diagnostic, like gf2_gather_cols_plan; out may be
 * NULL. */
int gf2_weights_plan(int what, int nrows, int ncols, long long out[4]);

#ifdef __cplusplus
}
#endif
#endif
