/* m4ri_hip_join_rows.h -- companion of m4ri_hip_find.h and m4ri_hip_join.h: the JOIN of two device pools on a column range of ANY width,
 * and the grouping of a pool by class that it rests on, ON THE DEVICE.  gf2_join_dev, gf2_join_select_dev, gf2_class_sort_dev and
 * gf2_lf2_reduce_dev match rows on a window of at most 30 bits; the upper levels of MMT / BJMM, the last merge of Wagner's k-list
 * algorithm, a whole-row meet in the middle and an LF2 round on a pool that has outgrown 2^30 classes match on 40 to 256 bits.
 * gf2_sort_rows_dev gives an order on such a range at ceil(width / 8) radix passes, gf2_find_rows_dev the lowest equal row and how many
 * there are; the entries here name the members of a class and walk them.  DESIGN.md section 7.22; INTEGRATION.md sections 3 and 4.
 *
 * value_M(i) = the columns [c0, c1) of row i of M, as in m4ri_hip_find.h.  0 <= c0 <= c1 <= ncols; c0 == c1: every value is 0.  Two rows
 * are in one CLASS when their values are equal; rep(i) is the lowest row j with value(j) == value(i).
 *
 * gf2_group_rows_dev:  order[s], 0 <= s < P->nrows, holds the rows of P in ascending order of (rep(i), i): the rows of a class are
 * contiguous and ascending, and the classes follow each other by their lowest row.  head[s] is the first sorted position of the class
 * of position s, as in gf2_sort_rows_dev; head may be NULL.  Both arrays are OVERWRITTEN: the caller zeroes nothing.  The classes are
 * exactly those of gf2_sort_rows_dev; only the order of the classes differs: order[head[s]] is the rep of gf2_unique_rows_dev for row
 * order[s], and the sizes of the classes are the mult of gf2_find_rows_dev(P, P, ...).  The call costs ceil(bits(nrows - 1) / 8) <= 4
 * radix passes whatever the width, against ceil((c1 - c0) / 8).  P->nrows == 0 writes nothing; c0 == c1 gives the identity order and
 * head all 0.
 *
 * gf2_join_rows_dev:  all pairs (i, j) with value_A(i) == value_B(j), ordered by (i, j) ascending -- the order of gf2_near_pairs_dev.
 * For t < min(*count, D->nrows):  D[t] = A[i] ^ B[j], ia[t] = i, ib[t] = j and wt[t] = the ones of D[t] in the columns [wc0, wc1).  ia, ib
 * and wt may each be NULL, independently.  *count (a DEVICE int64) is OVERWRITTEN with the number of all pairs: it may pass 2^31 and it
 * may pass the capacity.  D->nrows is the capacity; D->nrows == 0 is the count-only call; D->data == NULL with D->nrows > 0 is the
 * index-only mode of gf2_join_select_dev: the rows are not stored, the arrays are written.  Rows and entries from min(count, capacity)
 * on are not touched.  Rows of D are written whole by the rule of gf2_submatrix_dev: every word of the row width, the excess bits of
 * the last one zero.
 *
 * From gf2_join_dev:  A->ncols == B->ncols == D->ncols; 0 <= c0 <= c1 <= ncols and 0 <= wc0 <= wc1 <= ncols; A may be B, which gives all
 * ordered pairs of a class, (i, i) included; c0 == c1 means every row meets every row; an empty A or B gives *count = 0 and writes
 * nothing else.
 *
 * Equivalences.  (a) For c1 - c0 <= 30 the output is that of gf2_join_dev(D, A, B, c0, c1 - c0, ...) reordered by (ia, ib).  (b) For
 * c0 == c1 the output is bit for bit that of gf2_near_pairs_dev with flags == 0, wlo = 0 and whi = ncols.  (c) With A == B and i the
 * lowest row of its class, the ib of row i's pairs are the rows of that class in gf2_group_rows_dev's order.
 *
 * How it runs.  The table of gf2_find_rows_dev is filled and built over B and A is looked up in it: idx[i], the lowest partner, and
 * mult[i], how many there are.  The multiplicities are summed per run of 1024 rows, the run sums are scanned by one workgroup -- that
 * is *count, and where the count-only call ends, after five launches -- and every row gets the 64-bit offset of its first output.  B is
 * looked up in its own table, which gives rep; one launch writes the pairs (rep(j), j) and the stable 8-bit passes of the class sort
 * order them on bits(B->nrows - 1) bits (a pool of more than 2^30 rows in two chained windows); one launch over the sorted positions
 * writes the start of every class at its lowest row.  The scatter's grid runs over fixed chunks of 2048 OUTPUTS, sized by the capacity:
 * a workgroup leaves at once when its chunk lies behind min(count, capacity), finds its first and last row of A by bisection of the
 * offsets, stages that stretch of offsets in LDS (or bisects in global memory where the stretch is longer than a chunk) and deals its
 * outputs to lane groups sized by the row width; each output reads its row of B through the sorted order, forms the XOR with 16-byte
 * accesses where A, B and D each allow, takes the popcount on the weight range and stores.  One class of B->nrows members costs every
 * workgroup the same.  gf2_join_rows_plan names slots, form, passes, launches, chunk and scratch.
 *
 * Determinism.  Results do not depend on the order in which workgroups run: the table's kernels use integer atomics, but idx, mult and
 * rep do not depend on arrival order (m4ri_hip_find.h), and everything behind them is integer arithmetic with one writer per output
 * word, no atomics and no spins, flags or waits between workgroups.  Two calls give the same bits.
 *
 * What is read.  Nothing outside the ncols bits of a row; for the matching only the words of a row that hold a bit of [c0, c1), the
 * edge words through masks.  The words between the row width and `ld` are never read or written, so A, B and D may be strided views of
 * dirty parents.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word) are accepted: their words go one by one.
 * Rows are addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of P, A and B is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  All scratch -- the table, rep, class starts,
 * the sort's work space, the sorted order of B, idx and mult of A, offsets and run sums -- comes from the stream's scratch arena, from
 * a slot of its own; every scratch word that is read has been written by the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: the matrices (gf2_join_rows_dev: A, B, D, then their
 * widths), the range, then the arrays in the order of the arguments, then the weight range: a null matrix, a null `data` on a non-empty
 * matrix (D excepted), a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, widths that differ, a
 * range outside 0 <= c0 <= c1 <= ncols, a null `order` or `count`, a count that is not 8-byte aligned, an int array that is not 4-byte
 * aligned and a weight range outside 0 <= wc0 <= wc1 <= ncols return -1 and set gf2_last_error to a text that starts with the entry's
 * name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  gf2_group_rows_dev: the address ranges of order and head (P->nrows ints
 * each) may meet neither P's address range nor each other.  gf2_join_rows_dev, as gf2_join_dev: D may share no word with A or B (A and
 * B are only read and may overlap or be one view); the address ranges of count (one int64) and of ia, ib and wt (D->nrows ints each)
 * may meet neither A's, B's nor D's address range nor each other.  A D without data meets nothing. */
#ifndef M4RI_HIP_JOIN_ROWS_H
#define M4RI_HIP_JOIN_ROWS_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* value(i): the columns [c0, c1) of row i of P.  0 <= c0 <= c1 <= P->ncols.
 * order[s] (DEVICE int32[P->nrows], OVERWRITTEN): the rows of P ascending by (rep(i), i), rep(i) the lowest row with the value of row i.
 * head[s]  (may be NULL; DEVICE int32[P->nrows], OVERWRITTEN): the first sorted position of the class of position s. */
int gf2_group_rows_dev(gf2_dmat const *P, int c0, int c1, int *order, int *head, void *stream);

/* all pairs (i, j) with value_A(i) == value_B(j), by (i, j) ascending; for t < min(*count, D->nrows):
 * D[t] = A[i] ^ B[j] (D->data NULL: not stored), ia[t] = i, ib[t] = j, wt[t] = the ones of D[t] in [wc0, wc1) (DEVICE int32[D->nrows],
 * each may be NULL).  *count (DEVICE int64, OVERWRITTEN): the number of all pairs. */
int gf2_join_rows_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int c0, int c1, long long *count, int *ia, int *ib, int *wt,
                      int wc0, int wc1, void *stream);

/* without a device: returns the radix passes of the grouping of B, ceil(bits(nrows_b - 1) / 8) (0 for nrows_b <= 1), -1 for a bad shape
 * or a range outside 0 <= c0 <= c1 <= ncols.  out (may be NULL): out[0] = the slots of the table over B, out[1] = the form of its
 * kernels (0: a lane per row, 1: a wave per row, where the range holds more than 8 words), out[2] = the launches of
 * gf2_group_rows_dev on a pool of nrows_b rows with head == NULL (two more with head; 0 for nrows_b == 0), out[3] = the launches of
 * gf2_join_rows_dev with a capacity and something to write (the count-only call: 5; 0 where nrows_a == 0 or nrows_b == 0), out[4] =
 * the rows of A per workgroup of the sum and offset kernels (1024; the pair, start and head kernels take 256 rows), out[5] = the
 * outputs per workgroup of the scatter (2048), out[6] and out[7] = the scratch bytes of gf2_group_rows_dev and of gf2_join_rows_dev. */
int gf2_join_rows_plan(int nrows_a, int nrows_b, int ncols, int c0, int c1, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
