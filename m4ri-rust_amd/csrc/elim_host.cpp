// elim_host.cpp -- elimination on the device and its M4RI entry points: echelon forms, inverse, linear systems (kernels in gf2_elim.hip)
//   mzd_echelonize / _m4ri / _pluq   m4ri-sys/src/echelonform.rs:16-37, caller binary_matrix.rs:258-261
//   mzd_inv_m4ri                     m4ri-sys/src/brilliantrussian.rs:201-208, caller binary_matrix.rs:265-268
//   mzd_solve_left                   m4ri-sys/src/solve.rs:12-29, caller binary_matrix.rs:582-586
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "dev_args.h"
#include "gf2_kernels.h"
#include "gf2_env.h"

typedef uint64_t u64;

// In-place echelon form of the first `col_limit` columns of A (0 = all); row operations act on whole rows, so the
// columns beyond the limit carry an augmented right-hand side along.  full != 0: reduced row echelon form (unique);
// full == 0: pivot rows are only cleared below their column block.  Synchronous.  pivcols_dev (optional) receives a
// device array of the pivot columns that stays valid until `keep` is destroyed.
static int echelonize_dev(gf2_dmat *A, int full, int col_limit, int *rank_out, int *pivcols_host, DevBuf *pivcols_keep,
                   hipStream_t s) {
  const int m = A->nrows, ncols = A->ncols;
  const int limit = (col_limit > 0 && col_limit < ncols) ? col_limit : ncols;
  *rank_out = 0;
  if (m == 0 || limit == 0) return 0;
  const int kbw_env = env_int("M4RI_HIP_ELIM_BLOCK_WORDS", 32);  // read per call: tests shrink it
  const int KBW = kbw_env < 1 ? 1 : (kbw_env > 32 ? 32 : kbw_env);
  const long long aw = words_of(ncols), lw = words_of(limit), lda = A->ld;
  const int uw = KBW;
  const int max_rank = m < limit ? m : limit;
  const long long pld = (aw + 1) & ~1ll, tld = aw + uw;
  const int prow_max = m < KBW * 64 ? m : KBW * 64;

  DevBuf st, pivs, U, ptab, tmp, P, flags, blkpiv, moves;
  DevBuf &pv = pivcols_keep ? *pivcols_keep : pivs;
  if (int rc = st.alloc(sizeof(gf2k_elim_state))) return rc;
  if (int rc = pv.alloc((size_t)(max_rank + 64) * sizeof(int))) return rc;
  // small problems: one workgroup, the whole matrix in LDS.  It costs ~1 us per column it has to look at (it stops when
  // the rank reaches the row count) against ~0.8 us per column plus ~50 us fixed for the blocked algorithm below, so it
  // is taken when at most 256 columns can matter (1000 x 64: 94 us against 139; 10 x 10: 60 against 109)
  const int cols_to_visit = limit < m + 64 ? limit : m + 64;
  // (cols_to_visit is an estimate: a rank-deficient input walks all `limit` columns serially, hence the second bound)
  if (m <= 1024 && (long long)m * (aw | 1) <= 19000 && cols_to_visit <= 256 && limit <= 4096 && dev_env_int("M4RI_HIP_ELIM_SMALL", 1)) {
    HIP_TRY(gf2k_elim_small(A->data, lda, m, ncols, limit, full, reinterpret_cast<int *>(st.p), pv.as<int>(), s));
    HIP_TRY(hipMemcpyAsync(rank_out, st.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (pivcols_host && *rank_out > 0)
      HIP_TRY(hipMemcpyAsync(pivcols_host, pv.p, (size_t)*rank_out * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  }
  if (int rc = U.alloc((size_t)m * uw * sizeof(u64))) return rc;
  // the step's 64 pivot rows over the block + the 16 x 16 selector map + the stash of the next search (256 words, 256 flags: gf2_elim.hip)
  if (int rc = ptab.alloc((64 * 64 + 256 + 512) * sizeof(u64))) return rc;
  if (int rc = tmp.alloc((size_t)2 * GF2K_ELIM_BLOCK_PIVOTS * tld * sizeof(u64))) return rc;
  if (int rc = P.alloc((size_t)prow_max * pld * sizeof(u64))) return rc;
  if (int rc = flags.alloc((size_t)m)) return rc;
  if (int rc = blkpiv.alloc(GF2K_ELIM_BLOCK_PIVOTS * sizeof(int))) return rc;
  if (int rc = moves.alloc(4 * GF2K_ELIM_BLOCK_PIVOTS * sizeof(int))) return rc;
  gf2k_elim_state *dst = st.as<gf2k_elim_state>();
  HIP_TRY(hipMemsetAsync(dst, 0, sizeof(gf2k_elim_state), s));
  HIP_TRY(hipMemsetAsync(flags.p, 0, (size_t)m, s));

  // the pivot search of step j + 1 inside the update launch of step j (gf2_elim.hip, round 4); 0: two launches per step as before
  // (both switches are read by the shipped library too: a part or a partition on which the look-ahead launch cannot be resident as
  // a whole must be able to turn it off)
  static const int lookahead = env_int("M4RI_HIP_ELIM_LOOKAHEAD", 1);
  // test hook: 1 = update workgroup 0 of every look-ahead launch never raises its counters, so the look-ahead workgroup's bounded
  // wait runs out (tests/test_gpu_elim.py::test_lookahead_failure_is_reported_not_hung)
  static const int fault = env_int("M4RI_HIP_ELIM_FAULT", 0);
  const int full_and_flags = (full ? 1 : 0) | (fault << 8);
  // Without augmented columns (limit == ncols) the trailing product of a block does not wait for the block's result: it is
  // enqueued with what the host knows BEFORE the block -- the rank so far = the block's first pivot row r0 -- and with the largest
  // pivot count the block can have (the tracking columns of pivots that were not found are zero, so the rows of P they meet do
  // not matter); the record of the block comes back through pinned memory while the product runs.  The ~70 us per block the
  // device used to idle between the block's last kernel and the product's first (copy back, wake-up, a dozen launches) are gone:
  // 65536^2 59.1 -> 57.5 ms, 16384^2 8.2 -> 7.8, 4096^2 1.87 -> 1.81 (same box).  A block without pivots costs one wasted product, after which the next block
  // takes the waiting form; augmented systems (inverse, solve) keep it always: their product is cut at the last non-zero word.
  static const int spec_on = env_int("M4RI_HIP_ELIM_SPECULATE", 1);
  const bool spec = spec_on && limit == ncols;
  thread_local gf2k_elim_state *hpin = nullptr;
  thread_local std::map<int, hipEvent_t> hevs;  // one per device ORDINAL: an event belongs to the device that was current when it was created
  hipEvent_t hev = nullptr;
  if (spec) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (!hpin) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&hpin), sizeof(gf2k_elim_state), hipHostMallocPortable));
    hipEvent_t &slot = hevs[dev];
    if (!slot) HIP_TRY(hipEventCreateWithFlags(&slot, hipEventDisableTiming));
    hev = slot;
  }
  // Whatever way this function is left, the stream has drained before the scratch buffers above are handed back to the pool: an
  // error return behind an enqueued trailing product must not free U / P / tmp under it.  Declared after the buffers,
  // so destroyed before them.
  struct DrainOnExit {
    hipStream_t s;
    ~DrainOnExit() {
      if (hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
    }
  } drain{s};
  bool prev_empty = false;
  int r_cur = 0;
  for (long long c0w = 0; c0w < lw && r_cur < m; c0w += KBW) {
    const int sw = (int)(lw - c0w < KBW ? lw - c0w : KBW);
    const bool spec_now = spec && !prev_empty;
    HIP_TRY(hipMemsetAsync(U.p, 0, (size_t)m * uw * sizeof(u64), s));
    HIP_TRY(gf2k_elim_begin_block(dst, s));
    for (int j = 0; j < sw; ++j) {
      const bool last = (c0w + j == lw - 1) && (limit & 63);
      const u64 colmask = last ? ((1ull << (limit & 63)) - 1) : ~0ull;
      const bool last_next = (c0w + j + 1 == lw - 1) && (limit & 63);
      const u64 colmask_next = last_next ? ((1ull << (limit & 63)) - 1) : ~0ull;
      HIP_TRY(gf2k_elim_step(A->data, lda, m, c0w, sw, j, colmask, full_and_flags, U.as<u64>(), uw, uw, dst, pv.as<int>(),
                             ptab.as<u64>(), flags.as<unsigned char>(), blkpiv.as<int>(), colmask_next, lookahead, s));
    }
    HIP_TRY(gf2k_elim_end_block(A->data, lda, aw, c0w, U.as<u64>(), uw, uw, dst, flags.as<unsigned char>(), blkpiv.as<int>(),
                                moves.as<int>(), tmp.as<u64>(), tld, spec_now ? aw /* (no last-word scan) */ : c0w + sw, s));
    if (spec_now) {
      HIP_TRY(hipMemcpyAsync(hpin, dst, sizeof(gf2k_elim_state), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipEventRecord(hev, s));
      const int r0 = r_cur, rpmax = std::min(sw * 64, m - r0);
      const long long cR = c0w + sw;
      if (rpmax > 0 && cR < aw) {
        const int rows_lo = full ? 0 : r0;
        const int nright = ncols - (int)(cR * 64);
        HIP_TRY(hipMemcpy2DAsync(P.p, (size_t)pld * sizeof(u64), A->data + (long long)r0 * lda + cR, (size_t)lda * sizeof(u64),
                                 (size_t)(aw - cR) * sizeof(u64), rpmax, hipMemcpyDeviceToDevice, s));
        gf2_dmat Cw{A->data + (long long)rows_lo * lda + cR, lda, m - rows_lo, nright};
        gf2_dmat Uw{U.as<u64>() + (long long)rows_lo * uw, uw, m - rows_lo, rpmax};
        gf2_dmat Pw{P.as<u64>(), pld, rpmax, nright};
        if (int rc = gf2_mul_m4rm_plain(&Cw, &Uw, &Pw, 1, s)) return rc;
      }
      HIP_TRY(hipEventSynchronize(hev));  // the block's record (the product is running or queued behind it)
      if (hpin->err) return gf2_fail_msg("gf2 elimination: the look-ahead workgroup's wait for the update workgroups ran out");
      if (hpin->r0 != r0) return gf2_fail_msg("gf2 elimination: the device's rank record disagrees with the host's");
      prev_empty = hpin->r_cur == hpin->r0;
      r_cur = hpin->r_cur;
      continue;
    }
    gf2k_elim_state hst;
    HIP_TRY(hipMemcpyAsync(&hst, dst, sizeof(hst), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hst.err) return gf2_fail_msg("gf2 elimination: the look-ahead workgroup's wait for the update workgroups ran out");
    const int head[7] = {hst.r0, hst.r_cur, hst.np, hst.nmoves, hst.jbase, hst.scan, hst.lastword};
    const int r0 = head[0], rp = head[1] - head[0];
    r_cur = head[1];
    prev_empty = rp == 0;
    const long long cR = c0w + sw;
    const long long wlast = head[6];  // the block's pivot rows are zero beyond this word: so is their contribution
    if (rp > 0 && cR < aw && wlast >= cR) {
      // everything right of the block in one product: A[rows, right] ^= U'[rows, 0:rp] * (pivot rows of the block)
      const int rows_lo = full ? 0 : r0;
      const int nright = wlast == aw - 1 ? ncols - (int)(cR * 64) : (int)((wlast + 1 - cR) * 64);
      HIP_TRY(hipMemcpy2DAsync(P.p, (size_t)pld * sizeof(u64), A->data + (long long)r0 * lda + cR, (size_t)lda * sizeof(u64),
                               (size_t)(wlast + 1 - cR) * sizeof(u64), rp, hipMemcpyDeviceToDevice, s));
      gf2_dmat Cw{A->data + (long long)rows_lo * lda + cR, lda, m - rows_lo, nright};
      gf2_dmat Uw{U.as<u64>() + (long long)rows_lo * uw, uw, m - rows_lo, rp};
      gf2_dmat Pw{P.as<u64>(), pld, rp, nright};
      // plain M4RM on purpose: (a) the callers hold gf2_enqueue_mu, which mul_dispatch takes itself; (b) Strassen levels over
      // this shape (m x 2048 x n, through mul_strassen directly) were measured neutral: 85.7 against 85.3 ms at 65536^2 (round 3);
      // through the planner (GF2_ALGO_AUTO) again neutral in round 4: 58.58 against 58.56 ms, 16384^2 inverse 10.5 against 8.8
      if (int rc = gf2_mul_m4rm_plain(&Cw, &Uw, &Pw, 1, s)) return rc;
    }
  }
  *rank_out = r_cur;
  if (pivcols_host && r_cur > 0)
    HIP_TRY(hipMemcpyAsync(pivcols_host, pv.p, (size_t)r_cur * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gf2_echelonize_dev(gf2_dmat *A, int full, int ncols_limit, int *rank, int *pivot_cols, void *stream) {
  static const char fn[] = "gf2_echelonize_dev";
  if (int rc = gf2_check_mat(fn, "A", A)) return rc;
  GF2_RC(gf2_refuse_null(fn, "rank", rank));
  *rank = 0;
  if (A->nrows == 0 || A->ncols == 0) return 0;
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);
  return echelonize_dev(A, full, ncols_limit, rank, pivot_cols, nullptr, s);
}

int gf2_rref_keep_pivots_dev(gf2_dmat *A, int *rank, int *pivcols_host, void **pivcols_dev, size_t *pivcols_bytes, hipStream_t s) {
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);
  DevBuf pivs;
  if (int rc = echelonize_dev(A, 1, 0, rank, pivcols_host, &pivs, s)) return rc;
  *pivcols_dev = pivs.p;  // ownership moves to the caller
  *pivcols_bytes = pivs.bytes;
  pivs.p = nullptr;
  return 0;
}

// [ A | 0-pad to a word boundary | I ] -> reduced echelon form of the left part; singular unless rank == n
static int inverse_dev(gf2_dmat *Ainv, const u64 *Adata, long long lda, bool a_on_host, int n, int *singular, hipStream_t s) {
  const int nw = words_of(n);
  gf2_dmat T{nullptr, dev_ld_for(nw * 64 + n), n, nw * 64 + n};
  DevBuf tb;
  if (int rc = tb.alloc((size_t)n * T.ld * sizeof(u64))) return rc;
  T.data = tb.as<u64>();
  HIP_TRY(hipMemsetAsync(T.data, 0, (size_t)n * T.ld * sizeof(u64), s));
  HIP_TRY(hipMemcpy2DAsync(T.data, (size_t)T.ld * sizeof(u64), Adata, (size_t)lda * sizeof(u64), (size_t)nw * sizeof(u64), n,
                           a_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  HIP_TRY(gf2k_set_diag(T.data, T.ld, n, (long long)nw * 64, s));
  int rank = 0;
  if (int rc = echelonize_dev(&T, 1, n, &rank, nullptr, nullptr, s)) return rc;
  *singular = rank < n;
  if (rank == n) {
    HIP_TRY(hipMemcpy2DAsync(Ainv->data, (size_t)Ainv->ld * sizeof(u64), T.data + nw, (size_t)T.ld * sizeof(u64),
                             (size_t)nw * sizeof(u64), n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

extern "C" int gf2_inverse_dev(gf2_dmat *Ainv, gf2_dmat const *A, int *singular, void *stream) {
  static const char fn[] = "gf2_inverse_dev";
  if (gf2_check_mat(fn, "Ainv", Ainv) || gf2_check_mat(fn, "A", A)) return -1;
  GF2_RC(gf2_refuse_null(fn, "singular", singular));
  if (A->nrows != A->ncols || Ainv->nrows != A->nrows || Ainv->ncols != A->ncols)
    return gf2_bad_arg(fn, "matrices must be square and of equal size");
  *singular = 0;
  if (A->nrows == 0) return 0;
  // no aliasing rule: inverse_dev copies A into its scratch [A | pad | I] before anything is written, and writes Ainv from that
  // scratch when the elimination is over, so Ainv may be A or overlap it in any way
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);
  return inverse_dev(Ainv, A->data, A->ld, false, A->nrows, singular, s);
}

static int host_echelonize(mzd_t *A, int full, const char *name) {
  if (A->nrows == 0 || A->ncols == 0) return 0;
  gf2_cache_forget(A);  // modified in place
  auto bail = [&](const char *why) {
    std::fprintf(stderr, "m4ri_hip: %s failed: %s (%s)\n", name, why, gf2_last_error());
    std::abort();  // the M4RI signature has no error channel (returns the rank)
    return 0;
  };
  if (gf2_require_device()) return bail("no device");
  {
    const long long lim = gf2_small_work_limit();  // size dispatch, see host_mul_on
    if (lim > 0 && (long long)A->nrows * A->width * (A->nrows < A->ncols ? A->nrows : A->ncols) <= lim)
      return gf2_echelonize_host_small(A, full);
  }
  PinnedDevice pin;  // M4RI_HIP_DEVICES = one ordinal: run there
  hipStream_t s;
  if (gf2_private_stream(&s)) return bail("stream");
  int rank = 0, rc;
  {
    DMatOwner dA;
    rc = gf2_to_device(dA, A, s, true);
    if (!rc) rc = echelonize_dev(&dA.d, full, 0, &rank, nullptr, nullptr, s);
    if (!rc) rc = gf2_dmat_download(A, &dA.d, s);
    if (rc) (void)hipStreamSynchronize(s);
  }
  if (rc) return bail("device elimination");
  return rank;
}

extern "C" rci_t mzd_echelonize(mzd_t *A, int full) { return host_echelonize(A, full, "mzd_echelonize"); }
extern "C" rci_t mzd_echelonize_m4ri(mzd_t *A, int full, int k) {
  (void)k;  // table size hint of the CPU algorithm
  return host_echelonize(A, full, "mzd_echelonize_m4ri");
}
extern "C" rci_t mzd_echelonize_pluq(mzd_t *A, int full) { return host_echelonize(A, full, "mzd_echelonize_pluq"); }

extern "C" mzd_t *mzd_inv_m4ri(mzd_t *dst, mzd_t const *src, int k) {
  (void)k;
  if (src->nrows != src->ncols) gf2_die("mzd_inv_m4ri: matrix must be square.");
  if (dst && (dst->nrows != src->nrows || dst->ncols != src->ncols)) gf2_die("mzd_inv_m4ri: dst has wrong dimensions.");
  auto bail = [&](const char *why) -> mzd_t * {
    std::fprintf(stderr, "m4ri_hip: mzd_inv_m4ri failed: %s (%s)\n", why, gf2_last_error());
    return nullptr;
  };
  if (gf2_require_device()) return bail("no device");
  const int n = src->nrows;
  if (n == 0) return dst ? dst : mzd_init(0, 0);
  PinnedDevice pin;  // M4RI_HIP_DEVICES = one ordinal: run there
  hipStream_t s;
  if (gf2_private_stream(&s)) return bail("stream");
  int rc, singular = 0;
  const bool allocated = dst == nullptr;
  if (!dst) dst = gf2_mzd_init_uncleared(n, n);
  else gf2_cache_forget(dst);
  {
    DMatOwner dI;
    rc = gf2_to_device(dI, dst, s, false);
    if (!rc) rc = inverse_dev(&dI.d, src->rows[0], src->rowstride, true, n, &singular, s);
    if (!rc && !singular) rc = gf2_dmat_download(dst, &dI.d, s);
    if (rc) (void)hipStreamSynchronize(s);
  }
  if (rc || singular) {
    if (allocated) mzd_free(dst);
    if (rc) return bail("device elimination");
    return nullptr;  // not invertible: no inverse to return (callers see NULL; BinMatrix::inverted panics "Can't be NULL")
  }
  return dst;
}

// a system is inconsistent when a row below the rank of the reduced T = [ A | pad | B ] is non-zero in B's kb columns: *nonzero = 0 / 1
static int rhs_below_rank_nonzero(const gf2_dmat &T, int nw, int rank, int kb, int *nonzero, const char *what, hipStream_t s) {
  DevBuf flag;
  if (int rc = flag.alloc(sizeof(int))) return rc;
  int host = 0;
  hipError_t e = hipMemsetAsync(flag.p, 0, sizeof(int), s);
  if (e == hipSuccess) e = gf2k_any_nonzero(T.data + nw, T.ld, rank, T.nrows, kb, flag.as<int>(), s);
  if (e == hipSuccess) e = hipMemcpyAsync(&host, flag.p, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return gf2_fail_hip(e, what);
  *nonzero = host ? 1 : 0;
  return 0;
}

extern "C" int mzd_solve_left(mzd_t *A, mzd_t *B, int cutoff, int inconsistency_check) {
  (void)cutoff;
  if (A->ncols > B->nrows) gf2_die("mzd_solve_left: A ncols must be smaller than B nrows.");
  if (A->nrows > B->nrows) gf2_die("mzd_solve_left: A nrows must be smaller than B nrows.");
  const int m = A->nrows, n = A->ncols, kb = B->ncols;
  if (m == 0 || n == 0 || kb == 0) return 0;
  gf2_cache_forget(A);  // both are overwritten
  gf2_cache_forget(B);
  auto bail = [&](const char *why) {
    std::fprintf(stderr, "m4ri_hip: mzd_solve_left failed: %s (%s)\n", why, gf2_last_error());
    std::abort();  // -1 means "inconsistent" in this signature; a device failure is not that
    return -1;
  };
  if (gf2_require_device()) return bail("no device");
  PinnedDevice pin;  // M4RI_HIP_DEVICES = one ordinal: run there
  hipStream_t s;
  if (gf2_private_stream(&s)) return bail("stream");
  const int nw = words_of(n), bw = words_of(kb);
  int rc = 0, inconsistent = 0;
  do {
    // T = [ A | pad | B[0:m] ]
    gf2_dmat T{nullptr, dev_ld_for(nw * 64 + kb), m, nw * 64 + kb};
    DevBuf tb, xb, pivs;
    if ((rc = tb.alloc((size_t)m * T.ld * sizeof(u64)))) break;
    T.data = tb.as<u64>();
    hipError_t e = hipMemsetAsync(T.data, 0, (size_t)m * T.ld * sizeof(u64), s);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(T.data, (size_t)T.ld * sizeof(u64), A->rows[0], (size_t)A->rowstride * sizeof(word),
                           (size_t)nw * sizeof(u64), m, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(T.data + nw, (size_t)T.ld * sizeof(u64), B->rows[0], (size_t)B->rowstride * sizeof(word),
                           (size_t)bw * sizeof(u64), m, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      rc = gf2_fail_hip(e, "mzd_solve_left: upload");
      break;
    }
    int rank = 0;
    if ((rc = echelonize_dev(&T, 1, n, &rank, nullptr, &pivs, s))) break;
    if (inconsistency_check && rank < m && (rc = rhs_below_rank_nonzero(T, nw, rank, kb, &inconsistent, "mzd_solve_left: consistency check", s))) break;
    // X[pivot column k] = reduced right-hand side row k; free variables are 0; rows n.. of B are cleared
    gf2_dmat X{nullptr, dev_ld_for(kb), B->nrows, kb};
    if ((rc = xb.alloc((size_t)B->nrows * X.ld * sizeof(u64)))) break;
    X.data = xb.as<u64>();
    e = hipMemsetAsync(X.data, 0, (size_t)B->nrows * X.ld * sizeof(u64), s);
    if (e == hipSuccess) e = gf2k_scatter_rows(X.data, X.ld, T.data + nw, T.ld, bw, pivs.as<int>(), rank, s);
    if (e != hipSuccess) {
      rc = gf2_fail_hip(e, "mzd_solve_left: solution rows");
      break;
    }
    if ((rc = gf2_dmat_download(B, &X, s))) break;
    gf2_dmat Ared{T.data, T.ld, m, n};  // "A Input matrix (overwritten)": left holding its reduced echelon form
    if ((rc = gf2_dmat_download(A, &Ared, s))) break;
  } while (0);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return bail("device elimination");
  }
  return inconsistent ? -1 : 0;
}

// mzd_solve_left on device matrices: the same steps, with both uploads and the download of A replaced by block copies on the device
// and the solution rows scattered straight into B.
extern "C" int gf2_solve_left_dev(gf2_dmat *A, gf2_dmat *B, int check, int *inconsistent, void *stream) {
  if (!A || !B || !inconsistent) return gf2_fail_msg("gf2_solve_left_dev: null argument (A, B or inconsistent)");
  if (A->nrows < 0 || A->ncols < 0 || B->nrows < 0 || B->ncols < 0) return gf2_fail_msg("gf2_solve_left_dev: negative dimension");
  if (A->ncols > B->nrows) return gf2_fail_msg("gf2_solve_left_dev: A.ncols must not exceed B.nrows");
  if (A->nrows > B->nrows) return gf2_fail_msg("gf2_solve_left_dev: A.nrows must not exceed B.nrows");
  *inconsistent = 0;
  const int m = A->nrows, n = A->ncols, kb = B->ncols;
  if (m == 0 || n == 0 || kb == 0) return 0;
  if (!A->data || !B->data) return gf2_fail_msg("gf2_solve_left_dev: null argument (A.data or B.data)");
  const int nw = words_of(n), bw = words_of(kb);
  if (A->ld < nw || B->ld < bw) return gf2_fail_msg("gf2_solve_left_dev: row stride (A.ld or B.ld) smaller than row width");
  if ((reinterpret_cast<uintptr_t>(A->data) | reinterpret_cast<uintptr_t>(B->data)) & 7)
    return gf2_fail_msg("gf2_solve_left_dev: A.data or B.data is not 8-byte aligned");
  if ((long long)nw * 64 + kb > INT32_MAX) return gf2_fail_msg("gf2_solve_left_dev: A.ncols + B.ncols is too large");
  if (int rc = gf2_refuse_overlap("gf2_solve_left_dev", "B", B, "A", A)) return rc;  // both are written
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);
  int rc = 0;
  {
    // T = [ A | pad | B[0:m] ]
    gf2_dmat T{nullptr, dev_ld_for(nw * 64 + kb), m, nw * 64 + kb};
    DevBuf tb, pivs;
    do {
      if ((rc = tb.alloc((size_t)m * T.ld * sizeof(u64)))) break;
      T.data = tb.as<u64>();
      hipError_t e = hipMemsetAsync(T.data, 0, (size_t)m * T.ld * sizeof(u64), s);
      if (e != hipSuccess) {
        rc = gf2_fail_hip(e, "gf2_solve_left_dev: clearing the augmented matrix");
        break;
      }
      if ((rc = gf2_copy_block_dev(&T, 0, 0, A, 0, 0, m, n, 0, s))) break;
      if ((rc = gf2_copy_block_dev(&T, 0, nw * 64, B, 0, 0, m, kb, 0, s))) break;
      int rank = 0;
      if ((rc = echelonize_dev(&T, 1, n, &rank, nullptr, &pivs, s))) break;
      if (check && rank < m && (rc = rhs_below_rank_nonzero(T, nw, rank, kb, inconsistent, "gf2_solve_left_dev: consistency check", s))) break;
      // X[pivot column k] = reduced right-hand side row k; free variables are 0; every other row of B is cleared.  Whole words: the
      // excess bits of B's last word are zero before (a valid gf2_dmat) and after (T's are)
      e = gf2k_xor2d(B->data, B->ld, nullptr, 0, nullptr, 0, B->nrows, bw, s);
      if (e == hipSuccess) e = gf2k_scatter_rows(B->data, B->ld, T.data + nw, T.ld, bw, pivs.as<int>(), rank, s);
      if (e != hipSuccess) {
        rc = gf2_fail_hip(e, "gf2_solve_left_dev: solution rows");
        break;
      }
      gf2_dmat Ared{T.data, T.ld, m, n};  // A is left holding its reduced echelon form
      if ((rc = gf2_copy_block_dev(A, 0, 0, &Ared, 0, 0, m, n, 0, s))) break;
    } while (0);
    // the scratch goes back to the pool when this block ends: nothing queued may still use it
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "gf2_solve_left_dev: hipStreamSynchronize");
  }
  return rc;
}
