// ple_host.cpp -- mzp_t, the mzd_apply_p_* family, mzd_ple / mzd_pluq and mzd_pluq_solve_left (include/m4ri_hip.h; contract:
// INTEGRATION.md section 3).
//
// The factorisations and the solve run on the device (gf2_ple.hip) like mzd_echelonize does: upload, compute, download; a
// device failure aborts, because the M4RI signatures have no error channel.  Tiny matrices take gf2_ple_host_small and the host
// solve below, through the size dispatch of the drop-in entry points (gf2_small_host.cpp, M4RI_HIP_HOST_SMALL_WORK).  Both paths
// compute the same unique output: pivot rows = the row rank profile, ordered by pivot column; the other rows in their order.
// Permutations of host matrices are host work (row swaps, bit moves).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "api_internal.h"

namespace {

typedef unsigned long long u64;

inline int words_of(long long bits) { return (int)((bits + 63) >> 6); }
inline word high_mask(rci_t ncols) { return (ncols & 63) ? ((m4ri_one << (ncols & 63)) - 1) : m4ri_ffff; }
inline int get_bit(const word *row, int c) { return (int)((row[c >> 6] >> (c & 63)) & 1); }
inline void flip_bit(word *row, int c) { row[c >> 6] ^= m4ri_one << (c & 63); }

// host matrix -> dense words (width words per row, excess bits cleared)
std::vector<word> dense_of(const mzd_t *A) {
  const int w = words_of(A->ncols);
  std::vector<word> d((size_t)A->nrows * (w ? w : 1), 0);
  const word hm = high_mask(A->ncols);
  for (rci_t i = 0; i < A->nrows; ++i)
    for (int j = 0; j < w; ++j) d[(size_t)i * w + j] = j == w - 1 ? (A->rows[i][j] & hm) : A->rows[i][j];
  return d;
}

// dense words -> the rows of A, excess bits of each row's last word kept
void store_dense(mzd_t *A, const std::vector<word> &d) {
  const int w = words_of(A->ncols);
  const word hm = high_mask(A->ncols);
  for (rci_t i = 0; i < A->nrows; ++i)
    for (int j = 0; j < w; ++j) {
      const word v = d[(size_t)i * w + j];
      A->rows[i][j] = j == w - 1 ? ((A->rows[i][j] & ~hm) | (v & hm)) : v;
    }
}

// column permutations of at least this many bits go through the device (the threshold of mzd_transpose's device route)
constexpr long long kDeviceColPermBits = 1ll << 24;

// transposition list -> gather map (position i takes input index map[i])
std::vector<int> perm_map(const mzp_t *P, int n, bool descending) {
  std::vector<int> at(n);
  for (int i = 0; i < n; ++i) at[i] = i;
  const int len = P->length < n ? P->length : n;
  for (int t = 0; t < len; ++t) {
    const int i = descending ? len - 1 - t : t;
    const int j = P->values[i];
    if (j < 0 || j >= n) gf2_die("mzd_apply_p: permutation value out of range");
    std::swap(at[i], at[j]);
  }
  return at;
}

void apply_rows(mzd_t *A, const mzp_t *P, bool descending) {
  if (A->nrows == 0 || A->ncols == 0) return;
  gf2_cache_forget(A);
  const std::vector<int> map = perm_map(P, A->nrows, descending);
  std::vector<word> d = dense_of(A), out(d.size());
  const int w = words_of(A->ncols);
  for (rci_t i = 0; i < A->nrows; ++i) std::memcpy(&out[(size_t)i * w], &d[(size_t)map[i] * w], (size_t)w * sizeof(word));
  store_dense(A, out);
}

void apply_cols(mzd_t *A, const mzp_t *P, bool descending) {
  if (A->nrows == 0 || A->ncols == 0) return;
  gf2_cache_forget(A);
  const std::vector<int> map = perm_map(P, A->ncols, descending);  // validates P
  // large matrices: upload, transpose / row gather / transpose on the device, download (the bit loop below costs a host
  // operation per moved bit); the host loop stays the routine for small matrices and for a device call that failed
  if ((long long)A->nrows * A->ncols >= kDeviceColPermBits && gf2_device_count() > 0) {
    gf2_dmat d{nullptr, 0, 0, 0};
    if (gf2_dmat_alloc(&d, A->nrows, A->ncols) == 0) {
      int rc = gf2_dmat_upload(&d, A, nullptr);
      if (!rc) rc = gf2_apply_p_dev(&d, P->values, P->length, 1, descending ? 0 : 1, nullptr);
      if (!rc) rc = gf2_dmat_download(A, &d, nullptr);
      gf2_dmat_free(&d);
      if (!rc) return;
    }
  }
  std::vector<int> moved;
  for (int c = 0; c < A->ncols; ++c)
    if (map[c] != c) moved.push_back(c);
  if (moved.empty()) return;
  const int w = words_of(A->ncols);
  std::vector<word> tmp(w);
  for (rci_t i = 0; i < A->nrows; ++i) {
    word *row = A->rows[i];
    std::memcpy(tmp.data(), row, (size_t)w * sizeof(word));
    for (int c : moved)
      if (get_bit(row, c) != get_bit(tmp.data(), map[c])) flip_bit(row, c);
  }
}

// sigma[i] = input row at position i -> transposition list realising it under mzd_apply_p_left
void sigma_to_transpositions(const std::vector<int> &sigma, rci_t *P) {
  const int m = (int)sigma.size();
  std::vector<int> pos(m), at(m);
  for (int i = 0; i < m; ++i) pos[i] = at[i] = i;
  for (int i = 0; i < m; ++i) {
    const int p = pos[sigma[i]];
    P[i] = p;
    const int a = at[i], b = at[p];
    std::swap(at[i], at[p]);
    pos[a] = p;
    pos[b] = i;
  }
}

[[noreturn]] void device_failure(const char *name) {
  std::fprintf(stderr, "m4ri_hip: %s failed: device factorisation (%s)\n", name, gf2_last_error());
  std::abort();  // rci_t / int results have no error channel
}

bool small_ple(const mzd_t *A) {
  const long long lim = gf2_small_work_limit();
  const long long k = A->nrows < A->ncols ? A->nrows : A->ncols;
  return lim > 0 && (long long)A->nrows * words_of(A->ncols) * k <= lim;
}

rci_t host_ple(mzd_t *A, mzp_t *P, mzp_t *Q, int pluq, const char *name) {
  if (!A || !P || !Q) gf2_die((std::string(name) + ": null argument").c_str());
  if (P->length != A->nrows) gf2_die((std::string(name) + ": Length of P must match the number of rows of A.").c_str());
  if (Q->length != A->ncols) gf2_die((std::string(name) + ": Length of Q must match the number of columns of A.").c_str());
  for (rci_t i = 0; i < P->length; ++i) P->values[i] = i;
  for (rci_t i = 0; i < Q->length; ++i) Q->values[i] = i;
  if (A->nrows == 0 || A->ncols == 0) return 0;
  gf2_cache_forget(A);  // modified in place
  if (small_ple(A)) return gf2_ple_host_small(A, pluq, P->values, Q->values);
  gf2_dmat d{nullptr, 0, 0, 0};
  int rank = 0;
  if (gf2_dmat_alloc(&d, A->nrows, A->ncols)) device_failure(name);
  int rc = gf2_dmat_upload(&d, A, nullptr);
  if (!rc) rc = gf2_ple_dev(&d, pluq, P->values, Q->values, &rank, nullptr);
  if (!rc) rc = gf2_dmat_download(A, &d, nullptr);
  gf2_dmat_free(&d);
  if (rc) device_failure(name);
  return rank;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// mzp_t
// ---------------------------------------------------------------------------------------------------------------------

extern "C" mzp_t *mzp_init(rci_t length) {
  if (length < 0) gf2_die("mzp_init: negative length");
  mzp_t *P = static_cast<mzp_t *>(std::malloc(sizeof(mzp_t)));
  if (!P) gf2_die("out of memory");
  P->values = static_cast<rci_t *>(std::malloc(sizeof(rci_t) * (length ? length : 1)));
  if (!P->values) gf2_die("out of memory");
  P->length = length;
  for (rci_t i = 0; i < length; ++i) P->values[i] = i;
  return P;
}

extern "C" void mzp_free(mzp_t *P) {
  if (!P) return;
  std::free(P->values);
  std::free(P);
}

extern "C" mzp_t *mzp_init_window(mzp_t *P, rci_t begin, rci_t end) {
  if (!P || begin < 0 || end < begin || end > P->length) gf2_die("mzp_init_window: window out of range");
  mzp_t *W = static_cast<mzp_t *>(std::malloc(sizeof(mzp_t)));
  if (!W) gf2_die("out of memory");
  W->values = P->values + begin;
  W->length = end - begin;
  return W;
}

extern "C" void mzp_free_window(mzp_t *condemned) { std::free(condemned); }
extern "C" void Mzp_free_window(mzp_t *condemned) { mzp_free_window(condemned); }

extern "C" mzp_t *mzp_copy(mzp_t *P, mzp_t const *Q) {
  if (!Q) gf2_die("mzp_copy: source is NULL");
  if (!P) P = mzp_init(Q->length);
  else if (P->length < Q->length) gf2_die("mzp_copy: target is too short");
  if (P != Q && Q->length) std::memmove(P->values, Q->values, sizeof(rci_t) * Q->length);
  return P;
}

extern "C" void mzp_set_ui(mzp_t *P, unsigned int value) {
  if (value != 1) gf2_die("mzp_set_ui: only the identity (value 1) is supported");
  for (rci_t i = 0; i < P->length; ++i) P->values[i] = i;
}

extern "C" void mzp_print(mzp_t const *P) {
  std::printf("[");
  for (rci_t i = 0; i < P->length; ++i) std::printf(i ? " %d" : "%d", P->values[i]);
  std::printf("]\n");
  std::fflush(stdout);
}

extern "C" void mzd_apply_p_left(mzd_t *A, mzp_t const *P) { apply_rows(A, P, false); }
extern "C" void mzd_apply_p_left_trans(mzd_t *A, mzp_t const *P) { apply_rows(A, P, true); }
extern "C" void mzd_apply_p_right(mzd_t *A, mzp_t const *P) { apply_cols(A, P, true); }
extern "C" void mzd_apply_p_right_trans(mzd_t *A, mzp_t const *P) { apply_cols(A, P, false); }

// ---------------------------------------------------------------------------------------------------------------------
// PLE / PLUQ
// ---------------------------------------------------------------------------------------------------------------------

// Column-greedy elimination: the pivot of column c is the first remaining row (in input order) with bit c.  Any size; the
// drop-in entry points use it below the size dispatch.  P, Q: nrows / ncols ints.
extern "C" int gf2_ple_host_small(mzd_t *A, int pluq, int *P, int *Q) {
  const int m = A->nrows, n = A->ncols, w = words_of(n);
  for (int i = 0; i < m; ++i) P[i] = i;
  for (int j = 0; j < n; ++j) Q[j] = j;
  if (m == 0 || n == 0) return 0;
  std::vector<word> d = dense_of(A);
  const int kmax = m < n ? m : n, lw = words_of(kmax);
  std::vector<word> L((size_t)m * lw, 0);  // by input row
  std::vector<int> rest(m), order;
  for (int i = 0; i < m; ++i) rest[i] = i;
  for (int c = 0; c < n && !rest.empty(); ++c) {
    size_t at = 0;
    while (at < rest.size() && !get_bit(&d[(size_t)rest[at] * w], c)) ++at;
    if (at == rest.size()) continue;
    const int p = rest[at], k = (int)order.size();
    rest.erase(rest.begin() + (long)at);
    order.push_back(p);
    Q[k] = c;
    const word *e = &d[(size_t)p * w];
    for (int r : rest) {
      word *x = &d[(size_t)r * w];
      if (!get_bit(x, c)) continue;
      for (int j = c >> 6; j < w; ++j) x[j] ^= e[j];
      flip_bit(&L[(size_t)r * lw], k);
    }
  }
  const int rank = (int)order.size();
  std::vector<int> sigma(order);
  sigma.insert(sigma.end(), rest.begin(), rest.end());
  std::vector<word> out((size_t)m * (w ? w : 1), 0);
  for (int i = 0; i < m; ++i) {
    word *o = &out[(size_t)i * w];
    const word *l = &L[(size_t)sigma[i] * lw];
    const int nl = i < rank ? i : rank;  // L bits [0, nl)
    for (int k = 0; k < nl; ++k)
      if (get_bit(l, k)) flip_bit(o, k);
    if (i < rank) {
      std::vector<word> e(d.begin() + (long)sigma[i] * w, d.begin() + (long)(sigma[i] + 1) * w);
      if (pluq)  // U_i = E_i with the column transpositions of Q applied in ascending order
        for (int t = 0; t < rank; ++t)
          if (Q[t] != t && get_bit(e.data(), t) != get_bit(e.data(), Q[t])) {
            flip_bit(e.data(), t);
            flip_bit(e.data(), Q[t]);
          }
      for (int j = 0; j < w; ++j) o[j] |= e[j];
    }
  }
  store_dense(A, out);
  sigma_to_transpositions(sigma, P);
  return rank;
}

extern "C" rci_t mzd_ple(mzd_t *A, mzp_t *P, mzp_t *Q, int cutoff) {
  (void)cutoff;  // recursion cutoff of the CPU algorithm
  return host_ple(A, P, Q, 0, "mzd_ple");
}

extern "C" rci_t mzd_pluq(mzd_t *A, mzp_t *P, mzp_t *Q, int cutoff) {
  (void)cutoff;
  return host_ple(A, P, Q, 1, "mzd_pluq");
}

// ---------------------------------------------------------------------------------------------------------------------
// solve with a PLUQ factorisation
// ---------------------------------------------------------------------------------------------------------------------

namespace {

// P B, L^-1, the consistency test, U^-1, Q^T on dense copies (host routine of the size dispatch)
int pluq_solve_host(mzd_t const *A, rci_t r, mzp_t const *P, mzp_t const *Q, mzd_t *B, int check) {
  const int m = A->nrows, n = A->ncols, bw = words_of(B->ncols);
  std::vector<word> d = dense_of(B);
  auto row = [&](int i) { return &d[(size_t)i * bw]; };
  auto xor_row = [&](int i, int k) {
    word *a = row(i);
    const word *b = row(k);
    for (int j = 0; j < bw; ++j) a[j] ^= b[j];
  };
  const int plen = P->length < m ? P->length : m;
  for (int i = 0; i < plen; ++i)
    if (P->values[i] != i) std::swap_ranges(row(i), row(i) + bw, row(P->values[i]));
  for (int i = 0; i < r; ++i)
    for (int k = 0; k < i; ++k)
      if (get_bit(A->rows[i], k)) xor_row(i, k);
  int inconsistent = 0;
  if (check)
    for (int i = r; i < m && !inconsistent; ++i) {
      for (int k = 0; k < r; ++k)
        if (get_bit(A->rows[i], k)) xor_row(i, k);
      for (int j = 0; j < bw; ++j) inconsistent |= row(i)[j] != 0;
    }
  for (int i = r - 1; i >= 0; --i)
    for (int k = i + 1; k < r; ++k)
      if (get_bit(A->rows[i], k)) xor_row(i, k);
  std::fill(d.begin() + (long)r * bw, d.end(), 0);
  const int qlen = Q->length < n ? Q->length : n;
  for (int i = qlen - 1; i >= 0; --i)
    if (Q->values[i] != i) std::swap_ranges(row(i), row(i) + bw, row(Q->values[i]));
  store_dense(B, d);
  return inconsistent;
}

}  // namespace

extern "C" int mzd_pluq_solve_left(mzd_t const *A, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int cutoff, int check) {
  (void)cutoff;
  if (A->ncols > B->nrows) gf2_die("mzd_pluq_solve_left: A ncols must be smaller than B nrows.");
  if (A->nrows > B->nrows) gf2_die("mzd_pluq_solve_left: A nrows must be smaller than B nrows.");
  if (!P || !Q || P->length < A->nrows || Q->length < A->ncols) gf2_die("mzd_pluq_solve_left: P or Q too short.");
  if (rank < 0 || rank > A->nrows || rank > A->ncols) gf2_die("mzd_pluq_solve_left: rank out of range.");
  const int m = A->nrows, n = A->ncols, kb = B->ncols;
  if (m == 0 || n == 0 || kb == 0) return 0;
  gf2_cache_forget(B);
  int inconsistent = 0;
  const long long lim = gf2_small_work_limit();
  if (lim > 0 && (long long)(rank + 1) * (rank + 1 + m) * words_of(kb) <= lim) {
    inconsistent = pluq_solve_host(A, rank, P, Q, B, check);
  } else {
    gf2_dmat dA{nullptr, 0, 0, 0}, dB{nullptr, 0, 0, 0};
    int rc = gf2_dmat_alloc(&dA, m, n);
    if (!rc) rc = gf2_dmat_alloc(&dB, B->nrows, kb);
    if (!rc) rc = gf2_dmat_upload(&dA, A, nullptr);
    if (!rc) rc = gf2_dmat_upload(&dB, B, nullptr);
    if (!rc) rc = gf2_pluq_solve_left_dev(&dA, rank, P->values, Q->values, &dB, check, &inconsistent, nullptr);
    if (!rc) rc = gf2_dmat_download(B, &dB, nullptr);
    gf2_dmat_free(&dA);
    gf2_dmat_free(&dB);
    if (rc) device_failure("mzd_pluq_solve_left");
  }
  return (check && inconsistent) ? -1 : 0;
}
