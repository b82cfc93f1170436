// dev_args.h -- the argument and aliasing rules of the device-resident entries (include/m4ri_hip.h section 2 and the companion
// headers), one copy of each.  Everything here is plain host arithmetic: the entries check their arguments before a device is required
// and before the first HIP call, so a bad call fails the same way with and without a device.  The checks of one module alone (limits
// and texts of their own) stay with that module and are built from these.
#pragma once
#include <stdint.h>

#include <string>

#include "api_internal.h"

inline int gf2_bad_arg(const char *fn, const std::string &what) { return gf2_fail_msg((std::string(fn) + ": " + what).c_str()); }
// a pointer argument: "<name> is null", "<name> is not <N>-byte aligned" (align: a power of two).  Entries that accept a null pointer
// under some condition call the two halves on their own, in their own order.  (static, here and below: a helper that the library's
// table of exported symbols does not list already stays out of it)
static inline int gf2_refuse_null(const char *fn, const std::string &name, const void *p) {
  return p ? 0 : gf2_bad_arg(fn, name + " is null");
}
static inline int gf2_refuse_misaligned(const char *fn, const std::string &name, const void *p, int align) {
  if (!(reinterpret_cast<uintptr_t>(p) & (uintptr_t)(align - 1))) return 0;
  return gf2_bad_arg(fn, name + " is not " + std::to_string(align) + "-byte aligned");
}
static inline int gf2_check_ptr(const char *fn, const std::string &name, const void *p, int align) {
  if (int rc = gf2_refuse_null(fn, name, p)) return rc;
  return gf2_refuse_misaligned(fn, name, p, align);
}
// a matrix argument that can be addressed: `name` goes into the message.  unstored_ok: a null `data` on a non-empty matrix is accepted
// (gf2_subset_sums_dev: the rows are not stored, only the arrays that go with them are written); such a matrix shares no word with
// anything and meets no address range
inline int gf2_check_mat(const char *fn, const char *name, gf2_dmat const *M, bool unstored_ok = false) {
  const std::string n(name);
  GF2_RC(gf2_refuse_null(fn, n, M));
  if (M->nrows < 0 || M->ncols < 0) return gf2_bad_arg(fn, n + " has a negative dimension");
  if (M->nrows > 0 && M->ncols > 0 && !(unstored_ok && !M->data)) {
    GF2_RC(gf2_check_ptr(fn, n + ".data", M->data, 8));
    if (M->ld < (((long long)M->ncols + 63) >> 6))
      return gf2_bad_arg(fn, n + ".ld is smaller than the row width (the row stride cannot hold a row)");
  }
  return 0;
}
// the device check of an entry whose messages carry its name (the products answer with gf2_require_device's text)
static inline int gf2_require_device_for(const char *fn) { return gf2_device_count() > 0 ? 0 : gf2_bad_arg(fn, "no usable HIP device"); }
// what an entry returns after its last launch
static inline int gf2_hip_rc(hipError_t e, const char *what) { return e == hipSuccess ? 0 : gf2_fail_hip(e, what); }

// Do two rectangles of bits share a bit?  Rectangle X is xrows rows of xcols bits whose first bit has the bit address x0 (8 * byte
// address + bit in the word) and whose rows lie ldx words apart; Y likewise.  Both are non-empty and no wider than their stride.  With
// one stride a bit's address is row * L + column (L = 64 * ld), whatever parent the two views were cut from, so the answer is exact:
// with y0 - x0 = e L + f, 0 <= f < L, row j of Y starts f bits into row j + e of X and may run on into row j + e + 1.  With different
// strides the word ranges of the two rectangles are compared: conservative.
inline bool gf2_bit_rects_share(__int128 x0, long long ldx, long long xrows, long long xcols, __int128 y0, long long ldy, long long yrows,
                                long long ycols) {
  const __int128 L = (__int128)ldx * 64;
  if (ldx == ldy && L > 0 && xcols <= L && ycols <= L) {
    const __int128 x = y0 - x0;
    __int128 e = x / L, f = x % L;
    if (f < 0) {
      f += L;
      e -= 1;
    }
    const bool same = (e < xrows && -e < yrows) && f < xcols;
    const bool next = (e + 1 < xrows && -(e + 1) < yrows) && L - f < ycols;
    return same || next;
  }
  const __int128 x1 = x0 + ((__int128)(xrows - 1) * ldx) * 64 + xcols - 1, y1 = y0 + ((__int128)(yrows - 1) * ldy) * 64 + ycols - 1;
  return (x0 >> 6) <= (y1 >> 6) && (y0 >> 6) <= (x1 >> 6);
}
// "Do these two views share a word?": the rule above on the whole words of two matrices (an empty matrix shares nothing)
inline bool gf2_views_share_word(gf2_dmat const *X, gf2_dmat const *Y) {
  if (X->nrows <= 0 || X->ncols <= 0 || Y->nrows <= 0 || Y->ncols <= 0 || !X->data || !Y->data) return false;
  return gf2_bit_rects_share((__int128)reinterpret_cast<uintptr_t>(X->data) * 8, X->ld, X->nrows, (((long long)X->ncols + 63) >> 6) * 64,
                             (__int128)reinterpret_cast<uintptr_t>(Y->data) * 8, Y->ld, Y->nrows, (((long long)Y->ncols + 63) >> 6) * 64);
}
// one matrix under two names: what gf2_add_dev accepts as "in place"
inline bool gf2_same_view(gf2_dmat const *X, gf2_dmat const *Y) {
  return X->data == Y->data && X->ld == Y->ld && X->nrows == Y->nrows && X->ncols == Y->ncols;
}
// the refusal of a written matrix W that shares a word with another argument R of the call
inline int gf2_refuse_overlap(const char *fn, const char *w, gf2_dmat const *W, const char *r, gf2_dmat const *R) {
  if (!gf2_views_share_word(W, R)) return 0;
  return gf2_bad_arg(fn, std::string(w) + " and " + r + " overlap: " + w + " is written and may share no word with " + r +
                             " (with different ld: their address ranges may not meet)");
}

// Flat arrays (indices, weights, counts) know no rows: they are compared by address range, and so is a matrix against one of them --
// from its first word to the last word of its last row, the padding of the rows in between included.  An empty range meets nothing.
static inline bool gf2_ranges_meet(const void *p, long long pbytes, const void *q, long long qbytes) {
  const __int128 a0 = reinterpret_cast<uintptr_t>(p), a1 = a0 + pbytes;
  const __int128 b0 = reinterpret_cast<uintptr_t>(q), b1 = b0 + qbytes;
  return pbytes > 0 && qbytes > 0 && a0 < b1 && b0 < a1;
}
// one past the last byte of the words of a non-empty matrix
static inline __int128 gf2_mat_end(gf2_dmat const *M) {
  return (__int128)reinterpret_cast<uintptr_t>(M->data) + 8 * ((__int128)(M->nrows - 1) * M->ld + (((long long)M->ncols + 63) >> 6));
}
static inline bool gf2_range_meets_mat(const void *p, long long bytes, gf2_dmat const *M) {
  if (M->nrows <= 0 || M->ncols <= 0 || bytes <= 0 || !M->data) return false;
  const __int128 a0 = reinterpret_cast<uintptr_t>(p), a1 = a0 + bytes;
  return a0 < gf2_mat_end(M) && (__int128)reinterpret_cast<uintptr_t>(M->data) < a1;
}
// the int and count arrays of a call against its matrices and against each other: every array that is given (p != null) against
// every matrix, then against the arrays before it; "overlap" in the message
struct Gf2FlatArray {
  const char *name;
  const void *p;
  long long bytes;
};
struct Gf2NamedMat {
  const char *name;
  gf2_dmat const *m;
};
static inline int gf2_refuse_array_overlaps(const char *fn, const Gf2FlatArray *arrays, int n, const Gf2NamedMat *mats, int nmats) {
  for (int i = 0; i < n; ++i) {
    if (!arrays[i].p) continue;
    for (int k = 0; k < nmats; ++k)
      if (mats[k].m && gf2_range_meets_mat(arrays[i].p, arrays[i].bytes, mats[k].m))
        return gf2_bad_arg(fn, std::string(arrays[i].name) + " and " + mats[k].name + " overlap: the address range of " + arrays[i].name +
                                   " may not meet " + mats[k].name + "'s");
    for (int j = 0; j < i; ++j)
      if (arrays[j].p && gf2_ranges_meet(arrays[i].p, arrays[i].bytes, arrays[j].p, arrays[j].bytes))
        return gf2_bad_arg(fn, std::string(arrays[j].name) + " and " + arrays[i].name + " overlap: their address ranges may not meet");
  }
  return 0;
}
// ---- the rules that the LPN entries share (bkw, lf2, join, near, sums): one text each

// the key window [c0, c0 + b) of a call: its width, then its place in a matrix of ncols columns that the message calls `what` ("P",
// "A and B").  An entry with a check of its own between the two (gf2_join_dev) calls the halves in its own order
static inline int gf2_check_key_bits(const char *fn, int b, int maxb) {
  if (b < 0 || b > maxb) return gf2_bad_arg(fn, "b = " + std::to_string(b) + " is outside 0 <= b <= " + std::to_string(maxb));
  return 0;
}
static inline int gf2_check_key_columns(const char *fn, const char *what, int ncols, int c0, int b) {
  if (c0 < 0 || (long long)c0 + b > ncols)
    return gf2_bad_arg(fn, "the columns [c0, c0 + b) = [" + std::to_string(c0) + ", " + std::to_string((long long)c0 + b) + ") are outside " +
                               what + " (" + std::to_string(ncols) + " columns)");
  return 0;
}
static inline int gf2_check_key_window(const char *fn, const char *what, int ncols, int c0, int b, int maxb) {
  GF2_RC(gf2_check_key_bits(fn, b, maxb));
  return gf2_check_key_columns(fn, what, ncols, c0, b);
}
// the columns [wc0, wc1) whose ones are counted, in a matrix of ncols columns
static inline int gf2_check_weight_range(const char *fn, int ncols, int wc0, int wc1) {
  if (wc0 < 0 || wc0 > wc1 || wc1 > ncols)
    return gf2_bad_arg(fn, "the weight range [wc0, wc1) = [" + std::to_string(wc0) + ", " + std::to_string(wc1) + ") is outside 0 <= wc0 <= wc1 <= " +
                               std::to_string(ncols) + " columns");
  return 0;
}
// the weights [wlo, whi] that make a pair a hit
static inline int gf2_check_weight_window(const char *fn, int wlo, int whi) {
  if (wlo < 0 || wlo > whi)
    return gf2_bad_arg(fn, "the weight window [wlo, whi] = [" + std::to_string(wlo) + ", " + std::to_string(whi) + "] is outside 0 <= wlo <= whi");
  return 0;
}
// two pools and the matrix of their XORs: one width
static inline int gf2_check_equal_ncols(const char *fn, gf2_dmat const *A, gf2_dmat const *B, gf2_dmat const *D) {
  if (B->ncols != A->ncols || D->ncols != A->ncols)
    return gf2_bad_arg(fn, "A has " + std::to_string(A->ncols) + " columns, B " + std::to_string(B->ncols) + ", D " + std::to_string(D->ncols) +
                               ": A->ncols, B->ncols and D->ncols must be equal");
  return 0;
}

// two matrices by address range, whatever their strides (gf2_inverse_batch_dev: its kernel owns whole stacks)
static inline bool gf2_mat_ranges_meet(gf2_dmat const *X, gf2_dmat const *Y) {
  if (X->nrows <= 0 || X->ncols <= 0 || Y->nrows <= 0 || Y->ncols <= 0) return false;
  return (__int128)reinterpret_cast<uintptr_t>(X->data) < gf2_mat_end(Y) && (__int128)reinterpret_cast<uintptr_t>(Y->data) < gf2_mat_end(X);
}
