/* m4ri_hip_gather.h -- companion of m4ri_hip.h, section 2 (device-resident API): rows and columns of a device matrix selected by an
 * index array that lives ON THE DEVICE.  The pooled-Gauss round of an LPN solver (gather batch x k pool rows into a stack, concatenate
 * the right-hand side, gf2_echelonize_batch_dev) and the iteration of information-set decoding (a fresh column permutation or subset,
 * then an elimination) both stay on the caller's stream with these.  DESIGN.md section 7.8; INTEGRATION.md sections 3 and 4.
 *
 * These are gathers, not permutations: an index may occur any number of times, and D may have more or fewer rows (columns) than S.
 *
 * Index values.  -1 means "no source": a zero row or column (with `accumulate`: the destination row is left unchanged).  Any other
 * value outside [0, S->nrows) (rows) or [0, S->ncols) (columns) is treated as -1 and never dereferenced; if `bad` is non-NULL (a DEVICE
 * int that the caller has set to 0) a plain store -- not an atomic -- writes 1 there for such a value.  The calls never clear `bad`.
 * An EMPTY S with a non-empty D follows from this without a special case: D comes out zero (with `accumulate`: unchanged), and every
 * index other than -1 is out of range, so it COUNTS AS BAD and sets *bad.
 *
 * What is written.  Without `accumulate` D is written as a whole matrix, by the rule of gf2_submatrix_dev: the excess bits of its last
 * word come out zero whatever it held before, and a view keeps its neighbouring words.  With `accumulate` (rows only) only bits inside
 * D's columns change.  The excess bits of S's last word never reach the result, so S may be a view of a dirty parent.
 *
 * Alignment and ordering.  Both entries accept rows that are only 8-byte aligned (an odd `ld`, a base on an odd word); the row kernel
 * uses 16-byte accesses only where every row of D and S starts on a 16-byte boundary.  Both are asynchronous on `stream`, like
 * gf2_mul_dev: no host synchronisation and no hipMalloc; column gathers of a wide S (gf2_gather_cols_plan returns 1) take their scratch
 * from the stream's arena.
 *
 * Arguments are checked before a device is required and before the first HIP call: a null struct, a null `data` on a non-empty matrix,
 * a null `idx` with a non-empty D, a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned and a shape
 * mismatch return -1 and set gf2_last_error to a text that starts with the entry's name.  An empty D returns 0 without a device.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  D is written and may share no word with S -- decided on whole words as for
 * the other entries: exactly with equal `ld`, so D and S may be disjoint column ranges of one parent, and by address range with different
 * `ld`.  The address ranges of `idx` and of `bad` may not meet D's address range.  `idx` inside S is allowed: S is only read. */
#ifndef M4RI_HIP_GATHER_H
#define M4RI_HIP_GATHER_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* D[i] (^)= S[idx[i]] for i < D->nrows.  idx: DEVICE array of D->nrows int32.  D->ncols == S->ncols.
 * Aliasing: D may share no word with S (-1, "overlap"); idx and bad may not meet D's address range. */
int gf2_gather_rows_dev(gf2_dmat *D, gf2_dmat const *S, const int *idx, int accumulate, int *bad, void *stream);
/* D[r][j] = S[r][idx[j]] for j < D->ncols.  idx: DEVICE array of D->ncols int32.  D->nrows == S->nrows.
 * Aliasing: D may share no word with S (-1, "overlap"); idx and bad may not meet D's address range. */
int gf2_gather_cols_dev(gf2_dmat *D, gf2_dmat const *S, const int *idx, int *bad, void *stream);
/* which path a column gather of this shape takes, without a device: returns 0 = fused LDS kernel, 1 = composed route (transpose, row
 * gather, transpose through stream scratch), -1 = bad shape (a negative dimension);
 * out[0] = threads per workgroup, out[1] = LDS bytes per workgroup, out[2] = rows per workgroup, out[3] = scratch bytes.  Diagnostic,
 * like gf2_elim_batch_plan; out may be NULL. */
int gf2_gather_cols_plan(int nrows, int s_ncols, int d_ncols, long long out[4]);

#ifdef __cplusplus
}
#endif
#endif
