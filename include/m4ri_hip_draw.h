/* m4ri_hip_draw.h -- companion of m4ri_hip.h, section 2 (device-resident API): the DRAWS of a randomised solver ON THE DEVICE.  Every
 * randomised loop the library serves starts with one: the rows of each guess of a pooled-Gauss round (DISTINCT inside a guess, or the
 * system is singular), the column permutation of an information-set-decoding iteration, the Bernoulli(tau) noise of an LPN oracle.
 * With these entries such a loop has no host step left.  DESIGN.md section 7.14; INTEGRATION.md sections 3 and 4.
 *
 * The generator is Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC 2011; the Random123 library): counter-based, so a value is a function
 * of (seed, position) alone.  The draws are exact -- no floating point --, reproducible on the CPU bit for bit, positionable, and
 * Two runs give the same bits.  Multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds; the key
 * is (seed low 32, seed high 32); counter word 3 is a TAG that separates the entries: 1 Bernoulli, 2 indices, 3 subsets, 4
 * permutation.  Write x0..x3 for the output words and X for the 64-bit value x0 | x1 << 32.  A value in [0, n) is mulhi64(X, n), the
 * high 64 bits of the 128-bit product: exact and branch-free, with a bias below n / 2^64.
 *
 * gf2_bernoulli_dev / gf2_bernoulli_block_dev.  Every bit of D is 1 with probability thr / 2^32, independently.  The noise is a
 * function of (seed, thr, word index, bit) only, so a block drawn with row0, col_word0 and full_ncols equals the same rectangle of
 * the whole matrix; the three mean what they mean in gf2_dmat_fill_random_block: word j of row r of D is word
 *     widx = (row0 + r) * fullw + col_word0 + j
 * of the noise, fullw = the words of a row of full_ncols columns, or D's own width when full_ncols == 0.  For word widx, call q in
 * 0..15 is Philox(counter = (widx low, widx high, q, 1)) and yields the bit-planes R[2q] = x0 | x1 << 32, R[2q + 1] = x2 | x3 << 32.
 * Bit i of the 32-bit number U_i at bit-position m is bit i of R[m], and output bit i is U_i < thr.  (The kernel evaluates the
 * comparison bit-sliced and skips the calls that yield only planes below the lowest set bit of thr, which cannot change the outcome:
 * the calls made are q = ctz(thr) / 2 .. 15, two at thr = 2^29, sixteen at an odd thr.  thr == 0 makes no call.)
 * accumulate == 0 writes whole rows by the rule of gf2_submatrix_dev: the excess bits of the last word come out zero, and the words
 * between the row width and `ld` are never touched; D is never read.  accumulate != 0 XORs the noise into D; the noise word is
 * masked first, so excess bits stay as they were -- this is how noise goes into a label column.  Rows that are only 8-byte aligned
 * (an odd `ld`, a base on an odd word) are accepted; 16-byte stores are used only where every row allows it.  Rows are addressed
 * with 64-bit offsets.
 *
 * gf2_draw_indices_dev.  idx[t] = mulhi64(X_t, n), counter (t >> 1 low, t >> 1 high, 0, 2), X_t from (x0, x1) for even t and from
 * (x2, x3) for odd t: independent draws WITH replacement, which feed gf2_gather_rows_dev as they are.  1 <= n <= 2^31 - 1.
 * count == 0: nothing is written.
 *
 * gf2_draw_subsets_dev.  sub[g * k + t], g < batch, t < k: `batch` ordered k-tuples of DISTINCT values in [0, n), one per guess.
 * Each tuple is uniform over the injective tuples up to the bias of mulhi64; tuples are independent between subsets.  The rule is
 * deterministic and part of the contract.  In round a = 0, 1, ... every position t of subset g that is not yet settled draws
 *     v = mulhi64(X, n)   with counter ((g * k + t) low, high, a, 3)
 * and settles with v when (1) v is not the value of a position of g settled in an earlier round and (2) no unsettled position
 * t' < t of g drew the same v in this round: sequential rejection sampling replayed in (round, position) order.
 * 1 <= k <= 1024 and 2 k <= n, so every draw settles with probability 1/2 at least.  max_rounds == 0 means 64, otherwise
 * 1 <= max_rounds <= 64: the kernel is bounded in time by construction.  Positions still unsettled after max_rounds rounds read -1
 * (a zero row to the gathers); *unfinished, a DEVICE int32 that may be NULL, is OVERWRITTEN with the number of subsets that have
 * such a position.  At the default that has a probability of about k * 2^-64 per subset.  batch == 0: only *unfinished is written.
 *
 * gf2_draw_permutation_dev.  perm = the STABLE argsort of key(i) = x0 & (2^30 - 1), x0 from Philox(counter (i, 0, 0, 4)): a
 * permutation of 0 .. n - 1, unique, which feeds gf2_gather_cols_dev and gf2_gather_rows_dev as it is.  Ties fall in index order.
 * That is a deviation from the uniform permutation below n^2 / 2^31 in total variation (the chance that any two of the n keys
 * collide); where that matters, n is too large for this entry.  The sort is the class sort of m4ri_hip_lf2.h on (key, i) pairs,
 * four passes.  n == 0: nothing is written.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation and no hipMalloc.  Only the permutation needs work space (the
 * pair buffers and digit counts of its sort, gf2_draw_plan names the size): it comes from the stream's scratch arena, and every
 * scratch word that is read has been written by the same call.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null D, a null `data` on a non-empty matrix, a
 * negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned, a negative row0, col_word0 or full_ncols, a
 * block that does not fit the width of full_ncols, a null idx, sub or perm, an int array that is not 4-byte aligned, a negative
 * count or batch, n < 1 (the permutation: n < 0), k outside 1 <= k <= 1024, 2 k > n and max_rounds outside 0 .. 64 return -1 and
 * set gf2_last_error to a text that starts with the entry's name.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  The address range of sub (batch * k ints) may not meet that of
 * unfinished.  The other entries take one array. */
#ifndef M4RI_HIP_DRAW_H
#define M4RI_HIP_DRAW_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every bit of D (^)= 1 with probability thr / 2^32 (see above); the block form draws the rectangle at (row0, col_word0) of a
 * matrix of full_ncols columns (0: D's own width). */
int gf2_bernoulli_dev(gf2_dmat *D, uint32_t thr, uint64_t seed, int accumulate, void *stream);
int gf2_bernoulli_block_dev(gf2_dmat *D, uint32_t thr, uint64_t seed, int64_t row0, int64_t col_word0, int full_ncols, int accumulate,
                            void *stream);

/* idx: DEVICE int32[count], OVERWRITTEN with independent draws from [0, n). */
int gf2_draw_indices_dev(int *idx, long long count, int n, uint64_t seed, void *stream);

/* sub: DEVICE int32[batch * k], OVERWRITTEN with `batch` ordered k-tuples of distinct values from [0, n).  max_rounds: 0 (64) or
 * 1 .. 64.  unfinished: DEVICE int32 or NULL. */
int gf2_draw_subsets_dev(int *sub, int batch, int k, int n, uint64_t seed, int max_rounds, int *unfinished, void *stream);

/* perm: DEVICE int32[n], OVERWRITTEN with a permutation of 0 .. n - 1. */
int gf2_draw_permutation_dev(int *perm, int n, uint64_t seed, void *stream);

/* without a device: 0, or -1 for a bad `what` or shape.  out (may be NULL), by `what`:
 *   GF2_DRAW_BERNOULLI    out[0] = Philox calls per output word for thr, out[1] = threads per workgroup, out[2] = lanes of one pass
 *                         of the grid (a lane makes one word, or two where 16-byte stores are possible)
 *   GF2_DRAW_INDICES      count_or_k = count: out[0] = Philox calls in all, out[1] = threads per workgroup, out[2] = draws of one
 *                         pass of the grid
 *   GF2_DRAW_SUBSETS      count_or_k = k: out[0] = threads per workgroup, out[1] = LDS bytes of the kernel, out[2] = subsets per
 *                         workgroup, out[3] = the rounds of max_rounds == 0
 *   GF2_DRAW_PERMUTATION  out[0] = scratch bytes, out[1] = sort passes, out[2] = key bits */
#define GF2_DRAW_BERNOULLI 1
#define GF2_DRAW_INDICES 2
#define GF2_DRAW_SUBSETS 3
#define GF2_DRAW_PERMUTATION 4
int gf2_draw_plan(int what, long long count_or_k, int n, uint32_t thr, long long out[4]);

#ifdef __cplusplus
}
#endif
#endif
