/* m4ri_hip_unique.h -- companion of m4ri_hip_lf2.h: a STABLE SORT of the rows of a device matrix by ANY RANGE OF COLUMNS, and the
 * REMOVAL OF DUPLICATE ROWS on top of it, ON THE DEVICE.  gf2_class_sort_dev groups rows by a key of at most 30 bits.  The lists of
 * MMT / BJMM (the representation technique makes every solution many times), an LF2 pool after a few rounds and the lists of Wagner's
 * algorithm must keep ONE copy of every row, and two lists are compared as sets through a canonical order: both need the whole row,
 * or a window wider than 30 bits.  DESIGN.md section 7.20; INTEGRATION.md sections 3 and 4.
 *
 * value(i) = the integer whose bit j is column c0 + j of row i of P, 0 <= j < c1 - c0 (column c1 - 1 is the most significant bit): the
 * key of m4ri_hip_bkw.h / m4ri_hip_lf2.h without the limit of 30 bits.  0 <= c0 <= c1 <= P->ncols; c0 == c1: every value is 0.
 *
 * gf2_sort_rows_dev:  order[s], 0 <= s < P->nrows, are the rows of P sorted ascending by (value, row index): a STABLE sort by the
 * value, so ties come in ascending row order and the result is unique.  head[s] = the first sorted position of the class (the rows of
 * one value) that position s belongs to: head[s] <= s and head[head[s]] == head[s]; head may be NULL.  Both are OVERWRITTEN.
 * Equivalence with the class sort: for c1 - c0 <= 30, order equals what gf2_class_sort_dev(P, c0, c1 - c0, order, NULL, stream) writes,
 * bit for bit.
 *
 * gf2_unique_rows_dev:  row i is KEPT iff no row j < i has value(j) == value(i): the first occurrence of every distinct value.
 * keep[t], t < min(*count, cap), are the kept rows, ascending; entries behind that are not touched.  *count = the number of distinct
 * values; it may exceed cap.  keep may be NULL iff cap == 0: the count-only call, by which a caller sizes keep.  rep[i] = the lowest j
 * with value(j) == value(i), so rep[i] == i iff row i is kept; rep may be NULL.  count and rep are OVERWRITTEN: the caller zeroes
 * nothing.  keep feeds gf2_gather_rows_dev as it is: with keep preset to -1, the rows behind *count gather as zero.
 *
 * Empty inputs.  nrows == 0: *count = 0 and nothing else is written; gf2_sort_rows_dev writes nothing.  c0 == c1: order is the
 * identity, head is all 0, *count = 1, keep[0] = 0 and rep is all 0.
 *
 * How it runs.  The range is cut from c0 upward into windows of 24 columns, the last one taking what is left.  For every window,
 * least significant first, one launch writes pairs (the window's bits of a row, the row) in the current order, and the 8-bit passes of
 * the class sort run on those pairs; they are stable, so the chain is a sort by the whole range, in ceil((c1 - c0) / 8) passes.  The
 * heads come from comparing the rows at neighbouring sorted positions word by word, and a running maximum over the positions.  The
 * kept rows are an ascending compaction of one flag per row.  gf2_sort_rows_plan names windows, passes, launches and scratch.
 *
 * Determinism.  Results are exact and independent of the order in which workgroups run.  No atomics are used and there is one writer
 * per output word: Two runs give the same bits.
 *
 * What is read.  Only the words of a row that hold a bit of [c0, c1); the edge words are read through masks, so bits outside the range
 * never influence a result.  Excess bits and the words between the row width and `ld` are never read, so P may be a strided view of a
 * dirty parent.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word) are accepted; 16-byte accesses are used only
 * where every row of P starts on a 16-byte boundary (today: nowhere, a row's words are loaded one by one).  Rows are addressed with
 * 64-bit offsets, so operands past 4 GiB work.  Nothing of P is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  All work space -- (key, row) pairs in two
 * buffers, digit counts, one int per run of sorted positions, and for gf2_unique_rows_dev the sorted order, the heads, the flags and
 * the block counts of the compaction -- comes from the stream's scratch arena, from a slot of its own (gf2_sort_rows_plan names the
 * sizes); every scratch word that is read has been written by the same call.  A NULL head or rep costs the caller no array.
 *
 * Arguments are checked before a device is required and before the first HIP call, in the order of the arguments: a null P, a null
 * `data` on a non-empty matrix, a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, a range outside
 * 0 <= c0 <= c1 <= ncols, a null `order`, a null `count`, a null `keep` with cap > 0, a negative cap and an int array that is not 4-byte
 * aligned return -1 and set gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  The address ranges of order and head (P->nrows ints each), or of keep
 * (cap ints), count (one int) and rep (P->nrows ints), may meet neither P's address range nor each other. */
#ifndef M4RI_HIP_UNIQUE_H
#define M4RI_HIP_UNIQUE_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* order[s]: the rows of P ascending by (value, row index) -- a STABLE sort, unique result.
 * head (may be NULL): head[s] = the first sorted position of the class of position s (head[s] <= s, head[head[s]] == head[s]).
 * DEVICE int32[P->nrows] each, OVERWRITTEN. */
int gf2_sort_rows_dev(gf2_dmat const *P, int c0, int c1, int *order, int *head, void *stream);

/* Row i is KEPT iff no row j < i has value(j) == value(i) (the first occurrence of every distinct value).
 * keep[t], t < min(*count, cap): the kept rows, ascending; entries behind that are not touched.  keep may be NULL iff cap == 0.
 * *count (DEVICE int32, OVERWRITTEN): the number of distinct values; may exceed cap.
 * rep (may be NULL; DEVICE int32[P->nrows], OVERWRITTEN): rep[i] = the lowest j with value(j) == value(i); rep[i] == i iff i is kept. */
int gf2_unique_rows_dev(gf2_dmat const *P, int c0, int c1, int *keep, int cap, int *count, int *rep, void *stream);

/* without a device: returns the number of radix passes, ceil((c1 - c0) / 8) (0 for an empty range), -1 for a bad shape or a range
 * outside 0 <= c0 <= c1 <= ncols.  out (may be NULL): out[0] = windows, out[1] = bits per window (24; the last window takes what is
 * left), out[2] = radix passes, out[3] = launches of gf2_sort_rows_dev (3 more with head), out[4] = launches of gf2_unique_rows_dev
 * (one fewer with cap == 0), out[5] and out[6] = scratch bytes of each, out[7] = rows per run of the head kernels. */
int gf2_sort_rows_plan(int nrows, int ncols, int c0, int c1, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
