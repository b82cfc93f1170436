/* m4ri_hip_near.h -- companion of m4ri_hip_join_select.h: the HAMMING-DISTANCE SEARCH between two pools, ON THE DEVICE.  The joins pair
 * rows that are EQUAL on a window.  Here rows are paired that are CLOSE: the leaf of a nearest-neighbour search (May-Ozerov, Both-May),
 * the final check of Stern / MMT when the window is empty, "which codeword of this list is nearest to each received word", the removal
 * of near duplicates inside a pool.  All NA * NB pairs are weighed by a kernel that keeps its operands on chip (a row of A in registers,
 * tiles of B in LDS): XOR and popcount, bound by the vector units and not by two random row reads per pair as the join with b == 0 is.
 * DESIGN.md section 7.17; INTEGRATION.md sections 3 and 4.
 *
 * Write d(i, j) for the number of ones of A[i] ^ B[j] in the columns [wc0, wc1), A->ncols == B->ncols.  The ADMITTED pairs are all
 * (i, j) with 0 <= i < A->nrows and 0 <= j < B->nrows, minus those that `flags` excludes:
 *     GF2_NEAR_OFF_DIAGONAL   pairs with ia == ib are not admitted (A is B: a row is not its own neighbour)
 *     GF2_NEAR_UPPER          only pairs with ia < ib are admitted (A is B: every unordered pair once)
 * The flags compare row numbers alone: they may be given with A != B as well.  Unknown flag bits are refused.
 *
 * gf2_near_pairs_dev.  A pair is a HIT when it is admitted and wlo <= d(i, j) <= whi.  The h-th hit in the order (ia ascending, then ib
 * ascending) is written to
 *     D[h]  = A[ia] ^ B[ib]                                                   (the whole row, D->ncols == A->ncols)
 *     ia[h], ib[h] = its rows of A and of B,   wt[h] = d(ia, ib)              (ia, ib and wt may be NULL, independently)
 * for h < min(*hits, D->nrows); D->nrows is the capacity.  Nothing behind that is touched: rows of D, and entries of ia, ib and wt, from
 * min(*hits, capacity) on are not touched.  *hits = the number of all hits, a 64-bit integer: it may exceed 2^31, and *hits may exceed
 * the capacity.  It is OVERWRITTEN: the caller zeroes nothing.  A or B without rows: *hits = 0 and nothing else is written.
 *
 * Equivalence with the join.  With flags == 0 the results are bit for bit those of
 *     gf2_join_select_dev(D, A, B, 0, 0, wc0, wc1, wlo, whi, &count, hits, ia, ib, wt, stream)
 * (every row has key 0, the pairs ordered by (ia, ib)); count = NA * NB is not reported here.  The order is part of the contract.  No
 * atomics are used and there is one writer per output word: Two runs give the same bits.
 *
 * Modes.  D->data == NULL with D->nrows > 0 is allowed here, as in gf2_join_select_dev: the rows are not stored and only ia, ib and wt
 * (those that are given) are written for the first D->nrows hits.  This is the index-only mode.  D->nrows == 0 writes only *hits: the
 * counts-only call, by which a caller sizes D to exactly *hits rows.
 *
 * Weights and the window.  0 <= wc0 <= wc1 <= ncols, and 0 <= wlo <= whi; whi may exceed the width of the range.  An empty range
 * weighs 0, so every admitted pair is a hit when wlo == 0 and no pair otherwise.
 *
 * gf2_nearest_dev.  dist[i] = the minimum of d(i, j) over the admitted j, idx[i] = the lowest j that attains it.  A row with no
 * admitted partner gets idx[i] = -1 and dist[i] = -1: an empty B, GF2_NEAR_OFF_DIAGONAL with a B of one row (for row 0), every row from
 * B->nrows - 1 on under GF2_NEAR_UPPER.  idx and dist are DEVICE int32[A->nrows]; either may be NULL, not both; they are OVERWRITTEN.
 * The result is exact and does not depend on the order in which workgroups run: every chunk of B leaves the minimum of the keys
 * (d << 32 | j) of its pairs, and a second launch folds the chunks of a row.  An empty A writes nothing.
 *
 * What is written.  The rows [0, min(*hits, capacity)) of D are written as whole rows by the rule of gf2_submatrix_dev: the excess bits
 * of the last word are zero, and a view keeps its neighbouring words.
 *
 * What is read.  Only the ncols bits of the rows of A and B.  Excess bits and the words between the row width and `ld` are never read,
 * so A and B may be strided views of dirty parents.  Rows that are only 8-byte aligned are accepted; 16-byte accesses are used only
 * where every row of that operand starts on a 16-byte boundary (today: nowhere in global memory; the tiles of B in LDS are read 16
 * bytes at a time).  Rows are addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of A or B is written.  Every pair is
 * weighed twice at the most (once to count the hits of its cell, once more if its workgroup has a hit below the capacity) and only the
 * words that hold a column of the range are formed for it; a whole row is XORed for a hit alone.
 *
 * Asynchronous on `stream`: no host synchronisation and no hipMalloc.  The work space -- one int64 per row of A and chunk of B, the hit
 * counts of gf2_near_pairs_dev or the chunk minima of gf2_nearest_dev -- comes from the stream's scratch arena, from a slot of its own
 * (gf2_near_plan names the size, which does not grow with the number of pairs); every scratch word that is read has been written by
 * the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null A, B or D, a null `data` on a non-empty A or
 * B, a null `hits`, a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, a `hits` that is not 8-byte
 * aligned, an int array that is not 4-byte aligned, unequal column counts, a weight range outside 0 <= wc0 <= wc1 <= ncols, a weight
 * window outside 0 <= wlo <= whi, unknown flags and (gf2_nearest_dev) idx and dist both null return -1 and set gf2_last_error to a text
 * that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  A and B are only read: they may overlap or be the identical view (A may
 * be B: all ORDERED pairs, (i, i) included, unless the flags exclude them).  D may share no word with A or with B.  The address ranges
 * of hits (one int64), ia, ib and wt (D->nrows ints each) may meet none of the three matrices' address ranges, nor each other; those
 * of idx and dist (A->nrows ints each) may meet neither A's nor B's, nor each other.  A D without data meets nothing. */
#ifndef M4RI_HIP_NEAR_H
#define M4RI_HIP_NEAR_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GF2_NEAR_OFF_DIAGONAL 1 /* pairs with ia == ib are not admitted (A is B: a row is not its own neighbour) */
#define GF2_NEAR_UPPER 2        /* only pairs with ia < ib are admitted (A is B: every unordered pair once)      */

/* the admitted pairs whose XOR has wlo <= ones <= whi in the columns [wc0, wc1), ordered by (ia, ib) (see above).  D->nrows is the
 * capacity in hits (D->data NULL: the rows are not stored; D->nrows == 0: counts only).  hits: DEVICE int64.  ia, ib, wt: DEVICE
 * int32[D->nrows] each, or NULL (independently). */
int gf2_near_pairs_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int wc0, int wc1, int wlo, int whi, int flags,
                       long long *hits, int *ia, int *ib, int *wt, void *stream);

/* for every row of A the nearest admitted row of B on the columns [wc0, wc1): idx[i] the lowest such row, dist[i] its distance, both -1
 * where no row is admitted.  idx, dist: DEVICE int32[A->nrows] each, or NULL (not both). */
int gf2_nearest_dev(gf2_dmat const *A, gf2_dmat const *B, int wc0, int wc1, int flags, int *idx, int *dist, void *stream);

/* without a device: returns 0, or -1 for a bad shape or a weight range outside 0 <= wc0 <= wc1 <= ncols.  out (may be NULL): out[0] =
 * the kernel chosen: the words of the range it keeps in registers per row of A, 1, 2, 4, 8 or 16, and 0 for the wide kernel (a range of
 * more than 16 words, read from global memory), out[1] = threads per workgroup, out[2] = rows of A per workgroup, out[3] = the number
 * S of chunks that B is cut into, out[4] = rows of B per chunk, out[5] = LDS bytes, out[6] = scratch bytes (8 per row of A and chunk,
 * and 8 more), out[7] = the words of a row that hold a column of [wc0, wc1). */
int gf2_near_plan(int nrows_a, int nrows_b, int ncols, int wc0, int wc1, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
