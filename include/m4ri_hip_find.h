/* m4ri_hip_find.h -- companion of m4ri_hip_unique.h: the LOOKUP of every row of a device matrix A among the rows of a device matrix B,
 * through a HASH TABLE built from B, ON THE DEVICE.  gf2_join_dev pairs rows that agree on a window of at most 30 bits and
 * gf2_unique_rows_dev keeps one copy of every row; "is this row already in that list, and where?" is what every level of BKW / LF2,
 * MMT / BJMM and Wagner's algorithm asks next: a fresh level is filtered against the rows kept so far (a set difference), two lists are
 * intersected, a list is checked against a blacklist, a meet in the middle matches whole rows of 64 .. 256 bits, and class sizes are
 * wanted.  A lookup needs no order, only equality.  DESIGN.md section 7.21; INTEGRATION.md sections 3 and 4.
 *
 * value_M(i) = the columns [c0, c1) of row i of M, as in m4ri_hip_unique.h.  0 <= c0 <= c1 <= min(A->ncols, B->ncols); c0 == c1: every
 * value is 0.  A and B may have different ncols and ld.
 *
 * gf2_find_rows_dev:  idx[i], 0 <= i < A->nrows, is the LOWEST j with value_B(j) == value_A(i), -1 if there is none.  mult[i] is the
 * number of rows j of B with value_B(j) == value_A(i), 0 for a miss; mult may be NULL.  *count is the number of rows of A with
 * idx[i] >= 0; count may be NULL.  All three are OVERWRITTEN: the caller zeroes nothing.  idx feeds gf2_gather_rows_dev as it is (a
 * miss gathers as a zero row) and gf2_select_weights_dev, whose compare is signed: [-1, -1] selects the misses, [0, 2^31 - 1] the hits.
 *
 * A may be B.  Then idx is bit for bit the rep of gf2_unique_rows_dev(A, c0, c1, ...), and mult[i] is the size of row i's class.
 *
 * Empty inputs.  A->nrows == 0: *count = 0 and nothing else is written.  B->nrows == 0: idx is all -1, mult all 0, *count = 0, and no
 * table is made.  c0 == c1 with B->nrows > 0: idx is all 0, mult all B->nrows and *count = A->nrows.
 *
 * How it runs.  Three launches.  The first fills a table of `slots` entries, the lowest power of two >= 2 B->nrows, with "empty".  The
 * second hashes the masked range words of every row of B with a 64-bit mix and walks from slot (hash mod slots) linearly: an empty slot
 * is taken by compare-and-swap; a slot that holds an equal row keeps the lower of the two by an atomic minimum; any other slot is
 * passed.  Where the row ends, one is added to that slot's member count.  An entry keeps 32 bits of the hash beside the row, so most
 * unequal rows are passed without reading them.  The third hashes every row of A and walks the same way: the first empty slot is a
 * miss, a slot with an equal row the answer.  A range of up to 8 words is handled by a lane per row, a wider one by a wave per row whose
 * compare ends at the first 64 words that differ.  gf2_find_rows_plan names slots, scratch, launches and the form.
 *
 * Determinism.  Results are exact and independent of the order in which workgroups run, although the kernels use integer atomics, as
 * gf2_class_first_dev does: equal rows walk the same slots, an occupied slot never empties and its occupant only ever changes to an
 * equal row, so every class ends in exactly one slot, which holds its minimum and the sum of its ones.  The layout of the table may
 * depend on arrival order; idx, mult and count do not.  Two calls give the same bits.  No thread ever waits for another: there are no
 * spins, flags or locks, and every probe loop is bounded by `slots`.
 *
 * What is read.  Only the words of a row that hold a bit of [c0, c1); the edge words are read through masks, so bits outside the range
 * never influence hash or equality.  Excess bits and the words between the row width and `ld` are never read, so A and B may be strided
 * views of dirty parents.  Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word) are accepted: a row's words are loaded
 * one by one.  Rows are addressed with 64-bit offsets, so operands past 4 GiB work.  Nothing of A and B is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  The table -- 12 bytes per slot -- comes from the
 * stream's scratch arena, from a slot of its own; every scratch word that is read has been written by the same call.  A NULL mult or
 * count costs the caller no array.
 *
 * Arguments are checked before a device is required and before the first HIP call, in the order of the arguments: a null A or B, a
 * null `data` on a non-empty matrix, a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, a range
 * outside 0 <= c0 <= c1 <= min(A->ncols, B->ncols), a null `idx` and an int array that is not 4-byte aligned return -1 and set
 * gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  The address ranges of idx and mult (A->nrows ints each) and of count (one
 * int) may meet neither A's nor B's address range nor each other. */
#ifndef M4RI_HIP_FIND_H
#define M4RI_HIP_FIND_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* value_M(i): the columns [c0, c1) of row i of M, as in m4ri_hip_unique.h.  0 <= c0 <= c1 <= min(A->ncols, B->ncols).
 * idx[i]  (DEVICE int32[A->nrows], OVERWRITTEN): the LOWEST j with value_B(j) == value_A(i), -1 if there is none.
 * mult[i] (may be NULL; DEVICE int32[A->nrows], OVERWRITTEN): the number of rows j of B with value_B(j) == value_A(i) (0 for a miss).
 * *count  (may be NULL; DEVICE int32, OVERWRITTEN): the number of rows of A with idx[i] >= 0. */
int gf2_find_rows_dev(gf2_dmat const *A, gf2_dmat const *B, int c0, int c1, int *idx, int *mult, int *count, void *stream);

/* without a device: returns the table's slots (0 for nrows_b == 0; 2^31 - 1 where they are more: out[0] holds them in full), -1 for a
 * bad shape or a range outside 0 <= c0 <= c1 <= ncols.  out (may be NULL): out[0] = slots, out[1] = bytes per slot (12), out[2] = scratch
 * bytes, out[3] = launches (3; 0 where nrows_a == 0 or nrows_b == 0), out[4] and out[5] = rows per workgroup of the build and of the
 * lookup kernel, out[6] = the form (0: a lane per row, 1: a wave per row), out[7] = the words of a row that hold a column of the range. */
int gf2_find_rows_plan(int nrows_a, int nrows_b, int ncols, int c0, int c1, long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
