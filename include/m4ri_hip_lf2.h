/* m4ri_hip_lf2.h -- companion of m4ri_hip.h, section 2 (device-resident API): a STABLE SORT of the rows of a device matrix by a window
 * of bits, and the LF2 reduction of a BKW solver on top of it, ON THE DEVICE.  LF1 (m4ri_hip_bkw.h) XORs one representative into
 * the other members of its class and drops it, so every round costs 2^b samples.  LF2, the second algorithm of Levieil and Fouque,
 * XORs EVERY PAIR of rows inside a class: a pool of about 3 * 2^b rows keeps its size round after round.  A class of n members gives
 * n (n - 1) / 2 rows.  DESIGN.md section 7.13; INTEGRATION.md sections 3 and 4.
 *
 * The key is the key of m4ri_hip_bkw.h.  key(i) = bits [c0, c0 + b) of row i of P; bit j of the key is column c0 + j.  c0 may be any
 * bit offset: because b <= 30 the key spans at most two words of a row.  b == 0: every row has key 0, one class.
 *
 * gf2_class_sort_dev:  order[s], 0 <= s < P->nrows, are the rows of P sorted ascending by (key, row index): a STABLE sort by the key,
 * so ties come in ascending row order and the result is unique.  skeys[s] = key(order[s]); skeys may be NULL.  Both are OVERWRITTEN.
 * nrows == 0: nothing is written.  The sort is a radix sort written for this library (gf2_lf2_plan names its passes); grouping rows by
 * a window of bits is also the collision step of information-set decoding and of duplicate removal.
 *
 * gf2_lf2_reduce_dev, one LF2 round.  Let sigma = order as above, and for a sorted position s let t(s) be the first position of its
 * class.  The outputs are enumerated for s = 0, 1, ... and inside s for p = t(s), ..., s - 1; for each
 *     D[j]  = P[sigma(s)] ^ P[sigma(p)]
 *     lo[j] = sigma(p),  hi[j] = sigma(s)              (lo and hi may be NULL, independently)
 * Said another way: classes by ascending key, and inside a class the pairs of rows lo < hi ordered by (hi, lo).  The order is part of
 * the contract and unique: Two runs give the same bits.  *count = the sum over the classes of n (n - 1) / 2, a 64-bit integer: it may
 * exceed 2^31 and it may exceed D->nrows, which is the capacity.  D->nrows == 0 with D->data NULL is a count-only call.
 * nrows == 0: *count = 0 and nothing else is written.  All keys distinct: *count = 0 and no row is written.
 *
 * What is written.  Rows [0, min(count, capacity)) of D are written as whole rows by the rule of gf2_submatrix_dev: the excess bits
 * of the last word are zero, and a view keeps its neighbouring words.  Rows from min(count, capacity) on are not touched; the same
 * holds for lo and hi.  The window bits of D come out zero by construction.  count is OVERWRITTEN: the caller zeroes nothing.
 *
 * What is read.  Only the ncols bits of P's rows; gf2_class_sort_dev reads only the one or two words that hold the key (the second
 * only when the window crosses a word boundary, no word for b == 0).  Excess bits and the words between the row width and `ld` are
 * never read, so P may be a strided view of a dirty parent.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word)
 * are accepted; 16-byte accesses are used only where every row of P, and independently of D, starts on a 16-byte boundary.  Rows are
 * addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of P is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  All work space -- (key, row) pairs in two
 * buffers, digit counts, the sorted order and the run offsets of a round -- comes from the stream's scratch arena (gf2_lf2_plan names
 * the sizes); every scratch word that is read has been written by the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null P or D, a null `data` on a non-empty
 * matrix, a null D->data with D->nrows > 0, a null `order` or `count`, a negative dimension, an `ld` below the row width, a `data` that
 * is not 8-byte aligned, a `count` that is not 8-byte aligned, an int array that is not 4-byte aligned, a b outside 0 <= b <= 30, a
 * window [c0, c0 + b) outside P and D->ncols != P->ncols return -1 and set gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  D may share no word with P: there is no in-place round.  The address
 * ranges of order and skeys (P->nrows ints each), or of count (one int64), lo and hi (D->nrows ints each), may meet neither P's
 * address range, nor D's, nor each other. */
#ifndef M4RI_HIP_LF2_H
#define M4RI_HIP_LF2_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* order[s], 0 <= s < P->nrows: the rows of P sorted ascending by (key, row index) -- a STABLE sort by the key.
 * skeys[s] = key(order[s]), or skeys == NULL.  Both DEVICE int32[P->nrows], OVERWRITTEN. */
int gf2_class_sort_dev(gf2_dmat const *P, int c0, int b, int *order, int *skeys, void *stream);

/* One LF2 round (see above).  D->ncols == P->ncols; D->nrows is the capacity (0 with D->data NULL: a count-only call).
 * count: DEVICE int64.  lo, hi: DEVICE int32[D->nrows] each, or NULL (independently). */
int gf2_lf2_reduce_dev(gf2_dmat *D, gf2_dmat const *P, int c0, int b, long long *count, int *lo, int *hi, void *stream);

/* without a device: returns the number of sort passes (0 for b == 0), -1 for a bad shape.  out (may be NULL): out[0] = key bits per
 * pass, out[1] = threads per workgroup and out[2] = LDS bytes of the sort kernels, out[3] = rows per sort tile T, out[4] = rows per
 * run R of the pair kernels, out[5] = lanes per row of the pair scatter, out[6] = scratch bytes of gf2_class_sort_dev, out[7] =
 * scratch bytes of gf2_lf2_reduce_dev (those of its sort included). */
int gf2_lf2_plan(int nrows, int ncols, int b, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
