// blocks_host.cpp -- device-resident block copy, submatrix, concat and stack (include/m4ri_hip.h section 2; kernel: gf2_blocks.hip;
// DESIGN.md section 7.5).  Every argument is checked before the first HIP call, so a bad call fails the same way with and without a
// device, and an empty rectangle returns without one.
#include <stdint.h>

#include <string>

#include "dev_args.h"
#include "gf2_kernels.h"

namespace {

// Do the rectangles share a bit?  (Both are non-empty and lie inside their matrices.)  The rule is gf2_bit_rects_share's
// (dev_args.h): exact with one row stride, by word range with two.
bool rects_overlap(gf2_dmat const *D, long long dr, long long dc, gf2_dmat const *S, long long sr, long long sc, long long nrows,
                   long long ncols) {
  const __int128 s0 = (__int128)reinterpret_cast<uintptr_t>(S->data) * 8 + ((__int128)sr * S->ld) * 64 + sc;
  const __int128 d0 = (__int128)reinterpret_cast<uintptr_t>(D->data) * 8 + ((__int128)dr * D->ld) * 64 + dc;
  return gf2_bit_rects_share(s0, S->ld, nrows, ncols, d0, D->ld, nrows, ncols);
}

// 0: go ahead; 1: nothing to do; -1: refused (gf2_last_error is set)
int check_block(const char *fn, gf2_dmat const *D, int dr, int dc, gf2_dmat const *S, int sr, int sc, int nrows, int ncols) {
  if (gf2_check_mat(fn, "D", D) || gf2_check_mat(fn, "S", S)) return -1;
  if (dr < 0 || dc < 0 || sr < 0 || sc < 0 || nrows < 0 || ncols < 0) {
    const char *name = dr < 0 ? "dr" : dc < 0 ? "dc" : sr < 0 ? "sr" : sc < 0 ? "sc" : nrows < 0 ? "nrows" : "ncols";
    return gf2_bad_arg(fn, std::string(name) + " is negative");
  }
  if ((long long)sr + nrows > S->nrows || (long long)sc + ncols > S->ncols) return gf2_bad_arg(fn, "the rectangle leaves S");
  if ((long long)dr + nrows > D->nrows || (long long)dc + ncols > D->ncols) return gf2_bad_arg(fn, "the rectangle leaves D");
  if (nrows == 0 || ncols == 0) return 1;
  if (rects_overlap(D, dr, dc, S, sr, sc, nrows, ncols))
    return gf2_bad_arg(fn, "the rectangles of S and D overlap (or, with different ld, their address ranges do)");
  return 0;
}

// whole_matrix: the call writes D as a matrix (submatrix, concat, stack), so where it writes D's last column it also leaves the excess
// bits of that word zero, whatever D held before (a fresh gf2_dmat_alloc block is not cleared)
int launch(const char *fn, gf2_dmat *D, int dr, int dc, gf2_dmat const *S, int sr, int sc, int nrows, int ncols, int accumulate,
           bool whole_matrix, void *stream) {
  const int zero_tail = whole_matrix && dc + ncols == D->ncols;
  return gf2_hip_rc(gf2k_copy_block(D->data, D->ld, dr, dc, S->data, S->ld, sr, sc, nrows, ncols, accumulate, zero_tail,
                                    static_cast<hipStream_t>(stream)), fn);
}

}  // namespace

extern "C" int gf2_copy_block_dev(gf2_dmat *D, int dr, int dc, gf2_dmat const *S, int sr, int sc, int nrows, int ncols, int accumulate,
                                  void *stream) {
  static const char fn[] = "gf2_copy_block_dev";
  if (int rc = check_block(fn, D, dr, dc, S, sr, sc, nrows, ncols)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device_for(fn));
  return launch(fn, D, dr, dc, S, sr, sc, nrows, ncols, accumulate, false, stream);
}

extern "C" int gf2_submatrix_dev(gf2_dmat *D, gf2_dmat const *S, int lowr, int lowc, int highr, int highc, void *stream) {
  static const char fn[] = "gf2_submatrix_dev";
  if (gf2_check_mat(fn, "D", D) || gf2_check_mat(fn, "S", S)) return -1;
  if (lowr < 0 || lowc < 0 || highr < lowr || highc < lowc) return gf2_bad_arg(fn, "lowr / lowc / highr / highc do not describe a rectangle");
  if (D->nrows != highr - lowr || D->ncols != highc - lowc) return gf2_bad_arg(fn, "D must be (highr - lowr) x (highc - lowc)");
  if (int rc = check_block(fn, D, 0, 0, S, lowr, lowc, highr - lowr, highc - lowc)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device_for(fn));
  return launch(fn, D, 0, 0, S, lowr, lowc, highr - lowr, highc - lowc, 0, true, stream);
}

// two copies into one destination, both checked before the first is enqueued
static int two_blocks(const char *fn, gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, int br, int bc, void *stream) {
  const int ca = check_block(fn, C, 0, 0, A, 0, 0, A->nrows, A->ncols);
  if (ca < 0) return ca;
  const int cb = check_block(fn, C, br, bc, B, 0, 0, B->nrows, B->ncols);
  if (cb < 0) return cb;
  if (ca && cb) return 0;
  GF2_RC(gf2_require_device_for(fn));
  if (!ca)
    if (int rc = launch(fn, C, 0, 0, A, 0, 0, A->nrows, A->ncols, 0, true, stream)) return rc;
  if (!cb)
    if (int rc = launch(fn, C, br, bc, B, 0, 0, B->nrows, B->ncols, 0, true, stream)) return rc;
  return 0;
}

extern "C" int gf2_concat_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream) {
  static const char fn[] = "gf2_concat_dev";
  if (gf2_check_mat(fn, "C", C) || gf2_check_mat(fn, "A", A) || gf2_check_mat(fn, "B", B)) return -1;
  if (A->nrows != B->nrows) return gf2_bad_arg(fn, "A and B must have equal row counts (A.nrows != B.nrows)");
  if (C->nrows != A->nrows || (long long)C->ncols != (long long)A->ncols + B->ncols)
    return gf2_bad_arg(fn, "C must be A.nrows x (A.ncols + B.ncols)");
  return two_blocks(fn, C, A, B, 0, A->ncols, stream);
}

extern "C" int gf2_stack_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream) {
  static const char fn[] = "gf2_stack_dev";
  if (gf2_check_mat(fn, "C", C) || gf2_check_mat(fn, "A", A) || gf2_check_mat(fn, "B", B)) return -1;
  if (A->ncols != B->ncols) return gf2_bad_arg(fn, "A and B must have equal column counts (A.ncols != B.ncols)");
  if ((long long)C->nrows != (long long)A->nrows + B->nrows || C->ncols != A->ncols)
    return gf2_bad_arg(fn, "C must be (A.nrows + B.nrows) x A.ncols");
  return two_blocks(fn, C, A, B, A->nrows, 0, stream);
}
