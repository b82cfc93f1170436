/* m4ri_hip_sums.h -- companion of m4ri_hip.h, section 2 (device-resident API): SUBSET SUMS, all XORs of p rows of a matrix in rank
 * order, with the subsets and the Hamming weights of the sums, ON THE DEVICE.  These are the lists that a collision decoder joins
 * (m4ri_hip_join.h): Stern / Dumer with p columns per half, each list XORed with the syndrome; the base lists of MMT / BJMM and of
 * Wagner's algorithm; all p-subsets of the information set of Lee-Brickell; all secrets of weight p times A for the meet in the middle
 * of a sparse LPN secret.  DESIGN.md section 7.16; INTEGRATION.md sections 3 and 4.
 *
 * The order is part of the contract.  A subset of {0 .. n - 1} of size p is written ascending, c_1 < ... < c_p, and the subsets are
 * ordered colexicographically (by c_p, then c_(p-1), ..., then c_1).  The position of a subset in that order is its rank,
 *     rank(c) = C(c_1, 1) + C(c_2, 2) + ... + C(c_p, p)              (the combinatorial number system; p = 2: C(c_2, 2) + c_1)
 * The rank of a subset does not depend on n, so a list can be cut into windows of ranks, and a list over n rows is the beginning of
 * the list over n + 1.  1 <= p <= 4, and C(n, p) must not pass 2^62.
 *
 * gf2_subset_sums_dev.  n = S->nrows.  For t in [0, D->nrows), with (c_1 .. c_p) the subset of rank rank0 + t:
 *     D[t]              = base ^ S[c_1] ^ ... ^ S[c_p]                 (base: NULL, or a 1 x ncols matrix such as the syndrome)
 *     idx[t * p + i - 1] = c_i
 *     wt[t]             = the number of ones of D[t] in the columns [wc0, wc1)        (idx and wt may be NULL, independently)
 * 0 <= rank0 and rank0 + D->nrows <= C(n, p).  D->nrows == 0 is a success that writes nothing, and the only legal call when n < p.
 * S->ncols == D->ncols == base->ncols.
 *
 * Rows not stored.  D->data == NULL with D->nrows > 0 is legal here, and only here, when idx or wt is given: only those arrays are
 * written (with both NULL the call returns -1).  This is the Lee-Brickell mode: the weights of all C(n, p) candidates without a row of
 * D in memory; gf2_select_weights_dev picks the light ones and gf2_unrank_subsets_dev names them.
 *
 * Weights.  0 <= wc0 <= wc1 <= ncols; an empty range gives 0.  wt is an int32 array of D->nrows entries; gf2_select_weights_dev
 * (m4ri_hip_weight.h) takes it as it is, and its indices are ranks relative to rank0.
 *
 * What is written.  Rows [0, D->nrows) of D are written as whole rows by the rule of gf2_submatrix_dev: the excess bits of the last
 * word are zero, and a view keeps its neighbouring words.  idx gets D->nrows * p ints and wt D->nrows ints, nothing around them.  One
 * writer per word and no atomics: Two runs give the same bits.
 *
 * What is read.  Only the ncols bits of the rows of S and of base.  Excess bits and the words between the row width and `ld` are never
 * read, so S and base may be strided views of dirty parents.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word)
 * are accepted; 16-byte accesses are used only where every row of that operand -- S, base and D independently -- starts on a 16-byte
 * boundary.  Rows are addressed with 64-bit offsets, so D may lie past 4 GiB, and rank0 may pass 2^32.  Nothing of S or base is
 * written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  No scratch is needed (gf2_subset_sums_plan
 * says 0 bytes).
 *
 * Arguments are checked before a device is required and before the first HIP call: a null S or D, a null `data` on a non-empty S or
 * base, a base that is not one row, unequal column counts, a p outside 1 <= p <= 4, a C(n, p) that passes 2^62, a window of ranks
 * outside [0, C(n, p)], a weight range outside 0 <= wc0 <= wc1 <= ncols, a `data` that is not 8-byte aligned, an int array that is
 * not 4-byte aligned, an `ld` below the row width, a negative dimension and rows not stored with neither idx nor wt return -1 and set
 * gf2_last_error to a text that starts with the entry's name.  A call that has nothing to write returns 0 without a device.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  S and base are only read: they may overlap, for example base may be a row
 * of S's parent.  D may share no word with S or with base.  The address ranges of idx (D->nrows * p ints) and wt (D->nrows ints) may
 * meet none of the three matrices' address ranges, nor each other.
 *
 * gf2_unrank_subsets_dev.  idx[t * p + i - 1] = c_i of the subset of rank rank0 + ranks[t], for t in [0, count): the names of the hits
 * that gf2_select_weights_dev found among the weights of a window that began at rank0, or of ia[hit] / ib[hit] of a join of two lists.
 * ranks[t] == -1 gives p times -1: what gf2_select_weights_dev leaves behind *count in an idx that held -1 before (it does not touch
 * those entries), the value that the gathers read as "no row".  Any other rank0 + ranks[t] outside
 * [0, C(n, p)) gives p times -1 as well, is never used as an address, and is reported through `bad` by the convention of
 * gf2_gather_rows_dev: a DEVICE int that the caller has set to 0, into which a plain store writes 1; the call never clears it; it may
 * be NULL.  ranks: DEVICE int32[count]; idx: DEVICE int32[count * p]; 0 <= rank0 <= 2^62.  count == 0 is a success that writes
 * nothing.  Asynchronous on `stream`.  A null or misaligned ranks or idx, a misaligned bad, a negative count or n, a bad p, rank0 or
 * C(n, p) return -1; so do address ranges of ranks, idx and bad that meet ("overlap").
 *
 * Host routines of the order, without a device: gf2_subset_count, gf2_subset_rank, gf2_subset_unrank (below). */
#ifndef M4RI_HIP_SUMS_H
#define M4RI_HIP_SUMS_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* D[t] = base ^ S[c_1] ^ ... ^ S[c_p], (c_1..c_p) the subset of rank rank0 + t, for t in [0, D->nrows).
 * idx[t*p + i-1] = c_i;  wt[t] = ones of D[t] in the columns [wc0, wc1).  idx, wt: DEVICE int32 or NULL, independently.
 * base: NULL or a 1 x ncols matrix (the syndrome). */
int gf2_subset_sums_dev(gf2_dmat *D, gf2_dmat const *S, gf2_dmat const *base, int p, long long rank0, int *idx, int *wt, int wc0, int wc1,
                        void *stream);

/* idx[t*p ..] = the subset of rank rank0 + ranks[t]; ranks[t] == -1 -> p times -1 (what select_weights leaves behind *count);
 * any other rank outside [0, C(n,p)) -> p times -1, never used as an address, and reported through `bad` by the
 * convention of gf2_gather_rows_dev's `bad` (may be NULL). */
int gf2_unrank_subsets_dev(const int *ranks, int count, long long rank0, int p, int n, int *idx, int *bad, void *stream);

/* C(n, p); 0 for n < p; -1 for p outside 1..4 or a value past 2^62 */
long long gf2_subset_count(int n, int p);
/* host: the rank of c[0] < ... < c[p - 1]; -1 unless 0 <= c_1 < ... < c_p, 1 <= p <= 4 and the rank stays below 2^62 */
long long gf2_subset_rank(const int *c, int p);
/* host: c[0 .. p) = the subset of that rank; -1 for a bad rank (negative, 2^62 or more, or one whose c_p does not fit an int) or p */
int gf2_subset_unrank(long long rank, int p, int *c);

/* without a device: returns the id of the kernel that `count` sums of p of n rows of ncols columns run on, -1 for a bad shape (a
 * negative size, a p outside 1..4, a C(n, p) past 2^62, a count above C(n, p) or above 2^31 - 1).  Ids 0 .. 3: S is copied into LDS once
 * per workgroup, 1, 2, 8, 64 lanes per row; ids 4 .. 7: S is read from global memory (through L2), 1, 2, 8, 64 lanes per row.  p is a
 * kernel argument, not a template parameter: the ids do not depend on it.  out (may be NULL): out[0] = threads per workgroup, out[1] =
 * ranks per workgroup R, out[2] = lanes per row, out[3] = LDS bytes per workgroup (0: S from global memory), out[4] = workgroups,
 * out[5] = scratch bytes (0). */
int gf2_subset_sums_plan(int n, int ncols, int p, long long count, long long out[6]);

#ifdef __cplusplus
}
#endif
#endif
