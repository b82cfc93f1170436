// trsm_host.cpp -- mzd_trsm_lower_left / _upper_left / _lower_right / _upper_right (include/m4ri_hip.h; contract: INTEGRATION.md
// section 3).
//
// Like the factorisations of ple_host.cpp: work of at most M4RI_HIP_HOST_SMALL_WORK word operations (n * n * ceil(k / 64)) takes
// gf2_trsm_host_small below; everything else uploads T and B, runs gf2_trsm_dev (gf2_trsm.hip) and downloads B.  X is unique,
// so both paths give the same bits.  A device failure aborts: the M4RI signatures have no error channel.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "api_internal.h"

namespace {

inline int words_of(long long bits) { return (int)((bits + 63) >> 6); }
inline word low_bits(int n) { return n <= 0 ? 0 : (n >= 64 ? m4ri_ffff : ((m4ri_one << n) - 1)); }

// the strict triangle of T as dense words (w per row); the diagonal and the other triangle are never looked at
std::vector<word> clean_triangle(const mzd_t *T, bool upper) {
  const int n = T->nrows, w = words_of(n);
  std::vector<word> d((size_t)n * w, 0);
  for (int i = 0; i < n; ++i)
    for (int q = upper ? i >> 6 : 0; q < (upper ? w : (i >> 6) + 1); ++q) {
      const int lo = i - q * 64;  // bits of this word left of the diagonal
      const word m = upper ? (~low_bits(lo + 1) & low_bits(n - q * 64)) : low_bits(lo);
      if (m) d[(size_t)i * w + q] = T->rows[i][q] & m;
    }
  return d;
}

void check_dims(mzd_t const *T, mzd_t const *B, bool right, const char *name) {
  if (!T || !B) gf2_die((std::string(name) + ": null argument").c_str());
  if (T->nrows != T->ncols) gf2_die((std::string(name) + ": the triangular matrix must be square.").c_str());
  if ((right ? B->ncols : B->nrows) != T->nrows) gf2_die((std::string(name) + ": dimensions of B and the triangular matrix differ.").c_str());
}

void host_trsm(mzd_t const *T, mzd_t *B, bool upper, bool right, const char *name) {
  check_dims(T, B, right, name);
  const long long n = T->nrows, k = right ? B->nrows : B->ncols;
  if (n == 0 || B->nrows == 0 || B->ncols == 0) return;
  gf2_cache_forget(B);  // modified in place
  const long long lim = gf2_small_work_limit();
  if (lim > 0 && n * n * words_of(k) <= lim) {
    gf2_trsm_host_small(T, B, upper, right);
    return;
  }
  gf2_dmat dT{nullptr, 0, 0, 0}, dB{nullptr, 0, 0, 0};
  int rc = gf2_dmat_alloc(&dT, T->nrows, T->ncols);
  if (!rc) rc = gf2_dmat_alloc(&dB, B->nrows, B->ncols);
  if (!rc) rc = gf2_dmat_upload(&dT, T, nullptr);
  if (!rc) rc = gf2_dmat_upload(&dB, B, nullptr);
  if (!rc) rc = gf2_trsm_dev(&dT, &dB, upper, right, nullptr);
  if (!rc) rc = gf2_dmat_download(B, &dB, nullptr);
  gf2_dmat_free(&dT);
  gf2_dmat_free(&dB);
  if (rc) {
    std::fprintf(stderr, "m4ri_hip: %s failed: device solve (%s)\n", name, gf2_last_error());
    std::abort();
  }
}

}  // namespace

// Left: word-parallel row substitution (row i of X = row i of B plus the rows of X that T's row i names).  Right: per row x of
// B, once x_i is final, T's row i is added to the part of x that is still open (lower: i descending, upper: ascending).
extern "C" int gf2_trsm_host_small(mzd_t const *T, mzd_t *B, int upper, int right) {
  if (!T || !B || T->nrows != T->ncols || (right ? B->ncols : B->nrows) != T->nrows) return -1;
  gf2_note_host_small_call();
  const int n = T->nrows, tw = words_of(n), rows = B->nrows, bw = words_of(B->ncols);
  if (n == 0 || rows == 0 || B->ncols == 0) return 0;
  const std::vector<word> t = clean_triangle(T, upper != 0);
  const word hm = B->high_bitmask;
  std::vector<word> x((size_t)rows * bw);
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < bw; ++j) x[(size_t)i * bw + j] = j == bw - 1 ? (B->rows[i][j] & hm) : B->rows[i][j];
  if (!right) {
    for (int s = 0; s < n; ++s) {
      const int i = upper ? n - 1 - s : s;
      word *xi = &x[(size_t)i * bw];
      for (int q = 0; q < tw; ++q) {
        word bits = t[(size_t)i * tw + q];
        while (bits) {
          const int kk = q * 64 + __builtin_ctzll(bits);
          bits &= bits - 1;
          const word *xk = &x[(size_t)kk * bw];
          for (int j = 0; j < bw; ++j) xi[j] ^= xk[j];
        }
      }
    }
  } else {
    for (int r = 0; r < rows; ++r) {
      word *xr = &x[(size_t)r * bw];  // bw == tw
      for (int s = 0; s < n; ++s) {
        const int i = upper ? s : n - 1 - s;
        if (!((xr[i >> 6] >> (i & 63)) & 1)) continue;
        const word *ti = &t[(size_t)i * tw];
        for (int q = upper ? i >> 6 : 0; q < (upper ? tw : (i >> 6) + 1); ++q) xr[q] ^= ti[q];
      }
    }
  }
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < bw; ++j) {
      const word v = x[(size_t)i * bw + j];
      B->rows[i][j] = j == bw - 1 ? ((B->rows[i][j] & ~hm) | (v & hm)) : v;
    }
  return 0;
}

extern "C" void mzd_trsm_lower_left(mzd_t const *L, mzd_t *B, int cutoff) {
  (void)cutoff;  // recursion cutoff of the CPU algorithm
  host_trsm(L, B, false, false, "mzd_trsm_lower_left");
}

extern "C" void mzd_trsm_upper_left(mzd_t const *U, mzd_t *B, int cutoff) {
  (void)cutoff;
  host_trsm(U, B, true, false, "mzd_trsm_upper_left");
}

extern "C" void mzd_trsm_lower_right(mzd_t const *L, mzd_t *B, int cutoff) {
  (void)cutoff;
  host_trsm(L, B, false, true, "mzd_trsm_lower_right");
}

extern "C" void mzd_trsm_upper_right(mzd_t const *U, mzd_t *B, int cutoff) {
  (void)cutoff;
  host_trsm(U, B, true, true, "mzd_trsm_upper_right");
}
