/* m4ri_hip_bkw.h -- companion of m4ri_hip.h, section 2 (device-resident API): the BKW / LF1 reduction ON THE DEVICE.  A BKW solver
 * shortens its samples round by round: partition the pool by a window of b bits, XOR one representative of every class into the other
 * members of its class, drop the representative.  Every survivor then reads zero in the window.  After a rounds the pool is the
 * "reduced pool" that gf2_lpn_errors_dev and gf2_min_weight_dev (m4ri_hip_wht.h) score, so a whole solve is one chain on the caller's
 * stream.  DESIGN.md section 7.11; INTEGRATION.md sections 3 and 4.
 *
 * The reduction needs no sort.  The representative of a class is its row of LOWEST index: an unsigned integer minimum per class, so
 * it is exact, and the results do not depend on launch order or on how workgroups interleave.  Two runs give the same bits.  The
 * survivors keep their order (an ordered compaction, as in gf2_select_weights_dev).
 *
 * The key.  key(i) = bits [c0, c0 + b) of row i of P; bit j of the key is column c0 + j.  c0 may be any bit offset: because b <= 30
 * the key spans at most two words of a row.  b == 0: every row has key 0, one class.
 *
 * gf2_class_first_dev:  first[v] = the LOWEST row index i with key(i) == v, -1 if no row has that key.  first is OVERWRITTEN.
 *
 * gf2_lf1_reduce_dev, one LF1 round.  It computes `first` as gf2_class_first_dev does (first is work space AND output).  Row i
 * SURVIVES when first[key(i)] != i; with GF2_LF1_KEEP_ZERO every row with key 0 survives as well, unchanged (its window is zero
 * already).  With the survivors i_0 < i_1 < ...
 *     D[j]   = P[i_j] ^ P[first[key(i_j)]]          (KEEP_ZERO and key(i_j) == 0:  D[j] = P[i_j])
 *     src[j] = i_j                                    (src may be NULL)
 * for j < min(*count, D->nrows), and *count = the number of survivors in all, which may exceed D->nrows: D->nrows is the capacity.
 * D->nrows == 0 with D->data NULL is a count-only call.  nrows == 0: first is all -1 and *count = 0.
 *
 * What is written.  Rows [0, min(count, capacity)) of D are written as whole rows by the rule of gf2_submatrix_dev: the excess bits
 * of the last word are zero, and a view keeps its neighbouring words.  Rows from min(count, capacity) on are not touched; the same
 * holds for src.  The window bits of D come out zero by construction.  count and all 2^b entries of first are OVERWRITTEN: the caller
 * zeroes nothing.
 *
 * What is read.  Only the ncols bits of P's rows; gf2_class_first_dev reads only the one or two words that hold the key (the second
 * only when the window crosses a word boundary, no word for b == 0).  Excess bits and the words between the row width and `ld` are
 * never read, so P may be a strided view of a dirty parent.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word)
 * are accepted; 16-byte accesses are used only where every row of P, and independently of D, starts on a 16-byte boundary.  Rows are
 * addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of P is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  The block counts of the compaction come from
 * the stream's scratch arena (gf2_lf1_plan, out[4]); every scratch word that is read has been written by the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null P or D, a null `data` on a non-empty
 * matrix, a null D->data with D->nrows > 0, a null `first` or `count`, a negative dimension, an `ld` below the row width, a `data` that
 * is not 8-byte aligned, an int array that is not 4-byte aligned, a b outside 0 <= b <= 30, a window [c0, c0 + b) outside P, flag bits
 * other than GF2_LF1_KEEP_ZERO and D->ncols != P->ncols return -1 and set gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  D may share no word with P: there is no in-place round, because
 * representatives are read while survivors are written.  The address ranges of first (2^b ints), count (one int) and src (D->nrows
 * ints) may meet neither P's address range, nor D's, nor each other. */
#ifndef M4RI_HIP_BKW_H
#define M4RI_HIP_BKW_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GF2_LF1_KEEP_ZERO = 1 };

/* first[v] = the LOWEST row index i of P whose bits [c0, c0+b) read v (bit j of v is column c0 + j), -1 if no row does.
 * first: DEVICE int32[2^b], OVERWRITTEN. */
int gf2_class_first_dev(gf2_dmat const *P, int c0, int b, int *first, void *stream);

/* One LF1 round (see above).  D->ncols == P->ncols; D->nrows is the capacity (0 with D->data NULL: a count-only call).
 * first: DEVICE int32[2^b], work space AND output.  count: DEVICE int32.  src: DEVICE int32[D->nrows] or NULL. */
int gf2_lf1_reduce_dev(gf2_dmat *D, gf2_dmat const *P, int c0, int b, int flags, int *first, int *count, int *src, void *stream);

/* without a device: returns the variant of the class-first kernel (0: per-workgroup table in LDS, 1: atomics straight into first),
 * -1 for a bad shape; out[0] = threads per workgroup, out[1] = LDS bytes, out[2] = rows a workgroup of the count / scatter kernels
 * covers, out[3] = lanes per row of the scatter kernel, out[4] = scratch bytes from the stream's arena.  out may be NULL. */
int gf2_lf1_plan(int nrows, int ncols, int b, long long out[5]);

#ifdef __cplusplus
}
#endif
#endif
