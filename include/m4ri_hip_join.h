/* m4ri_hip_join.h -- companion of m4ri_hip.h, section 2 (device-resident API): the JOIN of two pools of rows on a window of bits, with
 * the Hamming weights of the XORs, ON THE DEVICE.  gf2_lf2_reduce_dev (m4ri_hip_lf2.h) XORs the pairs of rows of ONE pool whose windows
 * are equal; the algorithms that come after it match two DIFFERENT lists: the collision step of Stern / Dumer and of the MMT / BJMM
 * merges (all (i, j) with L1[i] and L2[j] equal on l bits, then the weight of L1[i] ^ L2[j] on the other rows), a merge of Wagner's
 * k-list algorithm, the meet in the middle for a sparse LPN secret.  DESIGN.md section 7.15; INTEGRATION.md sections 3 and 4.
 *
 * The key is the key of m4ri_hip_bkw.h and m4ri_hip_lf2.h.  key(i) = bits [c0, c0 + b) of a row; bit j of the key is column c0 + j.
 * c0 may be any bit offset: because b <= 30 the key spans at most two words of a row.  b == 0: every row has key 0, so every row of A
 * meets every row of B.  A->ncols == B->ncols == D->ncols, and the window lies at the same columns in A and in B.
 *
 * gf2_join_dev.  Let sigmaA and sigmaB be the stable class sorts of A and of B (gf2_class_sort_dev: ascending by (key, row index)),
 * and for a sorted position s of A let [l(s), u(s)) be the positions of sigmaB whose key is the key of s.  The outputs are enumerated
 * for s = 0, 1, ... and inside s for p = l(s), ..., u(s) - 1; for each
 *     D[t]  = A[sigmaA(s)] ^ B[sigmaB(p)]
 *     ia[t] = sigmaA(s),  ib[t] = sigmaB(p)
 *     wt[t] = the number of ones of D[t] in the columns [wc0, wc1)          (ia, ib and wt may be NULL, independently)
 * Said another way: classes by ascending key, and inside a class the pairs ordered by (ia, ib).  The order is part of the contract and
 * unique: Two runs give the same bits (no atomics, one writer per output word).  *count = the sum over the keys of nA(key) * nB(key),
 * a 64-bit integer: it may exceed 2^31 and it may exceed D->nrows, which is the capacity.  D->nrows == 0 with D->data NULL is a
 * count-only call.  A or B without rows: *count = 0 and nothing else is written.  No key in common: *count = 0 and no row is written.
 *
 * Weights.  0 <= wc0 <= wc1 <= ncols; an empty range gives 0.  The range may include the window, whose bits are zero in D by
 * construction.  wt is an int32 array of D->nrows entries; gf2_select_weights_dev (m4ri_hip_weight.h) takes it as it is, and its
 * indices, gathered from ia and ib, name the rows of A and B of every hit.
 *
 * What is written.  Rows [0, min(count, capacity)) of D are written as whole rows by the rule of gf2_submatrix_dev: the excess bits
 * of the last word are zero, and a view keeps its neighbouring words.  Rows from min(count, capacity) on are not touched; the same
 * holds for ia, ib and wt.  count is OVERWRITTEN: the caller zeroes nothing.
 *
 * What is read.  Only the ncols bits of the rows of A and B.  Excess bits and the words between the row width and `ld` are never read,
 * so A and B may be strided views of dirty parents.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word) are
 * accepted; 16-byte accesses are used only where every row of that operand -- A, B and D independently -- starts on a 16-byte
 * boundary.  Rows are addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of A or B is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  All work space -- the pair buffers and digit
 * counts of the two sorts, the sorted orders and keys of A and B, the run sums -- comes from the stream's scratch arena (gf2_join_plan
 * names the size); every scratch word that is read has been written by the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null A, B or D, a null `data` on a non-empty
 * matrix, a null D->data with D->nrows > 0, a null `count`, a negative dimension, an `ld` below the row width, a `data` that is not
 * 8-byte aligned, a `count` that is not 8-byte aligned, an int array that is not 4-byte aligned, a b outside 0 <= b <= 30, unequal
 * column counts, a window [c0, c0 + b) outside the columns and a weight range outside 0 <= wc0 <= wc1 <= ncols return -1 and set
 * gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  A and B are only read: they may overlap or be the identical view; such a
 * self-join yields all ORDERED pairs of a class, (i, i) included, which are zero rows.  D may share no word with A or with B.  The
 * address ranges of count (one int64), ia, ib and wt (D->nrows ints each) may meet none of the three matrices' address ranges, nor
 * each other. */
#ifndef M4RI_HIP_JOIN_H
#define M4RI_HIP_JOIN_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* all pairs (i, j), row i of A and row j of B, whose bits [c0, c0 + b) are equal (see above).  D->nrows is the capacity (0 with
 * D->data NULL: a count-only call).  count: DEVICE int64.  ia, ib, wt: DEVICE int32[D->nrows] each, or NULL (independently). */
int gf2_join_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int c0, int b, long long *count, int *ia, int *ib, int *wt, int wc0,
                 int wc1, void *stream);

/* without a device: returns the number of passes of either sort (0 for b == 0), -1 for a bad shape.  out (may be NULL): out[0] =
 * threads per workgroup, out[1] = sorted positions of A per run R, out[2] = lanes per row of the scatter, out[3] = the keys of B that
 * a workgroup stages in LDS at the most S (a longer span is bisected in global memory), out[4] = LDS bytes of the scatter kernel,
 * out[5] = scratch bytes of gf2_join_dev, out[6] = runs of A, out[7] = the share of out[5] that the two sorts work in. */
int gf2_join_plan(int nrows_a, int nrows_b, int ncols, int b, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
