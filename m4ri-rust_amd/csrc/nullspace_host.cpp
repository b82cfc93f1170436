// nullspace_host.cpp -- mzd_kernel_left_pluq and gf2_nullspace_host_small (include/m4ri_hip.h; contract: INTEGRATION.md section 3).
//
// Like mzd_echelonize: work of at most M4RI_HIP_HOST_SMALL_WORK word operations (rows * width * min(rows, cols)) takes
// gf2_nullspace_host_small below; everything else uploads A, runs gf2_nullspace_dev (gf2_nullspace.hip) and downloads the reduced
// echelon form and the basis.  The basis is unique (ascending free columns), so both paths give the same bits.  A device failure
// aborts: the M4RI signature has no error channel.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "api_internal.h"

namespace {

inline word low_bits(int n) { return n <= 0 ? 0 : (n >= 64 ? m4ri_ffff : ((m4ri_one << n) - 1)); }

// the six moves of a parallel-suffix compress under mask m (Hacker's Delight 7-4): they depend on the mask alone, and the column mask
// is the same for every row
struct Compress {
  word m = 0, mv[6] = {};
  int count = 0;
  explicit Compress(word mask) : m(mask), count(__builtin_popcountll(mask)) {
    word mm = mask, mk = ~mask << 1;
    for (int i = 0; i < 6; ++i) {
      word mp = mk ^ (mk << 1);
      mp ^= mp << 2;
      mp ^= mp << 4;
      mp ^= mp << 8;
      mp ^= mp << 16;
      mp ^= mp << 32;
      mv[i] = mp & mm;
      mm = (mm ^ mv[i]) | (mv[i] >> (1 << i));
      mk &= ~mp;
    }
  }
  word operator()(word x) const {
    x &= m;
    if (m == m4ri_ffff) return x;
    for (int i = 0; i < 6; ++i) {
      const word t = x & mv[i];
      x = (x ^ t) | (t >> (1 << i));
    }
    return x;
  }
};

}  // namespace

// A -> its reduced row echelon form; *K = the basis (n x (n - rank), mzd_init) or NULL for full column rank.  Returns the rank, -1
// for a null argument.
extern "C" int gf2_nullspace_host_small(mzd_t *A, mzd_t **K) {
  if (!A || !K) return -1;
  *K = nullptr;
  const int n = A->ncols, nw = A->width;
  const int r = gf2_echelonize_host_small(A, 1);  // counts the run (gf2_host_small_calls)
  const int d = n - r;
  if (d == 0) return r;
  // row i of the reduced form starts at its pivot column
  std::vector<word> pm(nw, 0);
  std::vector<int> piv(r);
  for (int i = 0, q = 0; i < r; ++i) {
    while (!(A->rows[i][q] & (q == nw - 1 ? A->high_bitmask : m4ri_ffff))) ++q;  // pivot columns ascend
    const int b = __builtin_ctzll(A->rows[i][q]);
    piv[i] = q * 64 + b;
    pm[q] |= m4ri_one << b;
  }
  std::vector<Compress> cx;
  cx.reserve(nw);
  for (int q = 0; q < nw; ++q) cx.emplace_back(~pm[q] & low_bits(n - q * 64));
  mzd_t *B = mzd_init(n, d);
  for (int i = 0; i < r; ++i) {
    word *out = B->rows[piv[i]];
    int pos = 0;
    for (int q = 0; q < nw; ++q) {
      if (!cx[q].count) continue;
      const word x = cx[q](A->rows[i][q]);
      const int sh = pos & 63;
      out[pos >> 6] |= x << sh;
      if (sh + cx[q].count > 64) out[(pos >> 6) + 1] |= x >> (64 - sh);
      pos += cx[q].count;
    }
  }
  for (int q = 0, j = 0; q < nw; ++q)
    for (word f = cx[q].m; f; f &= f - 1, ++j) B->rows[q * 64 + __builtin_ctzll(f)][j >> 6] |= m4ri_one << (j & 63);
  *K = B;
  return r;
}

extern "C" mzd_t *mzd_kernel_left_pluq(mzd_t *A, int cutoff) {
  (void)cutoff;  // recursion cutoff of the CPU algorithm
  if (!A) gf2_die("mzd_kernel_left_pluq: null argument");
  const long long m = A->nrows, n = A->ncols;
  if (n == 0) return nullptr;
  gf2_cache_forget(A);  // modified in place
  auto bail = [&](const char *why) {
    std::fprintf(stderr, "m4ri_hip: mzd_kernel_left_pluq failed: %s (%s)\n", why, gf2_last_error());
    std::abort();
  };
  if (gf2_device_count() <= 0) bail("no device");
  mzd_t *K = nullptr;
  const long long lim = gf2_small_work_limit();
  if (lim > 0 && m * A->width * (m < n ? m : n) <= lim) {
    gf2_nullspace_host_small(A, &K);
    return K;
  }
  gf2_dmat dA{nullptr, 0, 0, 0}, dK{nullptr, 0, 0, 0};
  int rank = 0;
  int rc = gf2_dmat_alloc(&dA, A->nrows, A->ncols);
  if (!rc && m > 0) rc = gf2_dmat_upload(&dA, A, nullptr);
  if (!rc) rc = gf2_nullspace_dev(&dA, &dK, &rank, nullptr, nullptr);
  if (!rc && m > 0) rc = gf2_dmat_download(A, &dA, nullptr);
  if (!rc && dK.data) {
    K = mzd_init(dK.nrows, dK.ncols);
    rc = gf2_dmat_download(K, &dK, nullptr);
  }
  gf2_dmat_free(&dA);
  gf2_dmat_free(&dK);
  if (rc) bail("device null space");
  return K;
}
