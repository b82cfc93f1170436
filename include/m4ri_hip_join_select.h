/* m4ri_hip_join_select.h -- companion of m4ri_hip_join.h: the WEIGHT-FILTERED JOIN of two pools, ON THE DEVICE.  In every list decoder
 * that gf2_join_dev serves (Stern / Dumer, the MMT / BJMM merges, Wagner's merges, the meet in the middle for a sparse secret) the join
 * is followed by a weight test that almost no pair passes.  gf2_join_dev writes every pair and its weight, gf2_select_weights_dev reads
 * the weights again and the gathers pick out a handful of rows: the capacity, an int, and the memory are priced by the PAIRS.  Here only
 * the light pairs leave the kernel: the capacity is priced by the HITS, and a join of more than 2^31 pairs can be examined at all.
 * DESIGN.md section 7.15.1; INTEGRATION.md sections 3 and 4.
 *
 * gf2_join_select_dev.  The key, the window [c0, c0 + b) with b <= 30 (the key spans at most two words of a row), b == 0 (every row
 * has key 0) and A->ncols == B->ncols == D->ncols are those of gf2_join_dev.  The pairs are those of gf2_join_dev, in its order: with
 * the stable class sorts sigmaA and sigmaB, for s = 0, 1, ... and inside s for p = l(s), ..., u(s) - 1 the pair t = (sigmaA(s),
 * sigmaB(p)) -- classes by ascending key, and inside a class the pairs ordered by (ia, ib).  Write w(t) for the number of ones of
 * A[ia] ^ B[ib] in the columns [wc0, wc1).  A pair is a HIT when wlo <= w(t) <= whi.  The h-th hit in that order is written to
 *     D[h]  = A[ia] ^ B[ib]
 *     ia[h], ib[h] = its rows of A and of B,   wt[h] = w(t)                  (ia, ib and wt may be NULL, independently)
 * for h < min(*hits, D->nrows); D->nrows is the capacity.  Nothing behind that is touched: rows of D, and entries of ia, ib and wt, from
 * min(*hits, capacity) on are not touched.  *count = the number of all pairs, the same number as gf2_join_dev; *hits = the number of all
 * hits.  Both are 64-bit integers: each may exceed 2^31, and *hits may exceed the capacity.  Both are OVERWRITTEN: the caller zeroes
 * nothing.  A or B without rows, or no key in common: *count = 0, *hits = 0 and nothing else is written.
 *
 * Equivalence with the composed route.  The results are bit for bit those of gf2_join_dev with enough capacity (D->nrows >= count, the
 * same wc0 and wc1), followed by gf2_select_weights_dev(wt, count, wlo, whi, ...) and the gathers of D, ia, ib and wt by its indices.
 * The order is part of the contract.  No atomics are used and there is one writer per output word: Two runs give the same bits.
 *
 * Modes.  D->data == NULL with D->nrows > 0 is allowed here, as in gf2_subset_sums_dev: the rows are not stored and only ia, ib and wt
 * (those that are given) are written for the first D->nrows hits.  This is the index-only mode.  D->nrows == 0 writes only *count and
 * *hits: the counts-only call, by which a caller sizes D to exactly *hits rows.
 *
 * Weights and the window.  0 <= wc0 <= wc1 <= ncols, and 0 <= wlo <= whi; whi may exceed the width of the range.  An empty range
 * weighs 0, so every pair is a hit when wlo == 0 and no pair otherwise.  The range may include the key's window, whose bits are zero
 * in every pair.
 *
 * What is written.  The rows [0, min(*hits, capacity)) of D are written as whole rows by the rule of gf2_submatrix_dev: the excess bits
 * of the last word are zero, and a view keeps its neighbouring words.
 *
 * What is read.  Only the ncols bits of the rows of A and B.  Excess bits and the words between the row width and `ld` are never read,
 * so A and B may be strided views of dirty parents.  Rows that are only 8-byte aligned are accepted; 16-byte accesses are used only
 * where every row of that operand -- A, B and D independently -- starts on a 16-byte boundary.  Rows are addressed with 64-bit offsets,
 * so operands past 4 GiB work.  Nothing of A or B is written.  Every pair is weighed twice at the most (once to count the hits of its
 * run of A, once more if that run has a hit below the capacity) and only the words that hold a column of the range are formed for it;
 * a whole row is XORed for a hit alone.
 *
 * Asynchronous on `stream`, like gf2_join_dev: no host synchronisation and no hipMalloc.  All work space -- that of gf2_join_dev and
 * the hit sums, two int64 per run of A -- comes from the stream's scratch arena, from the slot of gf2_join_dev (gf2_join_select_plan
 * names the size, which does not grow with the number of pairs); every scratch word that is read has been written by the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null A, B or D, a null `data` on a non-empty A or
 * B, a null `count` or `hits`, a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, a `count` or
 * `hits` that is not 8-byte aligned, an int array that is not 4-byte aligned, a b outside 0 <= b <= 30, unequal column counts, a window
 * [c0, c0 + b) outside the columns, a weight range outside 0 <= wc0 <= wc1 <= ncols and a weight window outside 0 <= wlo <= whi return
 * -1 and set gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  A and B are only read: they may overlap or be the identical view (A may
 * be B: all ORDERED pairs of a class, (i, i) included).  D may share no word with A or with B.  The address ranges of count and hits
 * (one int64 each), ia, ib and wt (D->nrows ints each) may meet none of the three matrices' address ranges, nor each other.  A D
 * without data meets nothing. */
#ifndef M4RI_HIP_JOIN_SELECT_H
#define M4RI_HIP_JOIN_SELECT_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the pairs of gf2_join_dev(A, B, c0, b) whose XOR has wlo <= ones <= whi in the columns [wc0, wc1), in the join's order (see above).
 * D->nrows is the capacity in hits (D->data NULL: the rows are not stored; D->nrows == 0: counts only).  count, hits: DEVICE int64.
 * ia, ib, wt: DEVICE int32[D->nrows] each, or NULL (independently). */
int gf2_join_select_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int c0, int b, int wc0, int wc1, int wlo, int whi,
                        long long *count, long long *hits, int *ia, int *ib, int *wt, void *stream);

/* without a device: returns the number of passes of either sort (0 for b == 0), -1 for a bad shape or a weight range outside
 * 0 <= wc0 <= wc1 <= ncols.  out (may be NULL): out[0] = threads per workgroup, out[1] = sorted positions of A per run R, out[2] = lanes
 * per pair of the weigh pass (by the words of a row that hold a column of [wc0, wc1)), out[3] = lanes per row of the row store (by the
 * row width), out[4] = LDS bytes of the scatter kernel, out[5] = scratch bytes of gf2_join_select_dev (those of gf2_join_dev and the
 * hit sums), out[6] = runs of A, out[7] = outputs per round of the scatter G = out[0] / out[3]. */
int gf2_join_select_plan(int nrows_a, int nrows_b, int ncols, int b, int wc0, int wc1, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
