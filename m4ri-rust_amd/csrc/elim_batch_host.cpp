// elim_batch_host.cpp -- batched elimination of small matrices on the device (include/m4ri_hip.h section 2: gf2_echelonize_batch_dev,
// gf2_inverse_batch_dev, gf2_elim_batch_plan; kernels: gf2_elim_batch.hip).  Like blocks_host.cpp, every
// argument is checked before a device is required and before the first HIP call, so a bad call fails the same way with and without
// a device.  A call is one kernel launch on the caller's stream: no host synchronisation, no allocation.
#include <stdint.h>

#include <string>

#include "dev_args.h"
#include "gf2_kernels.h"

namespace {

constexpr int kMaxRows = 512, kMaxCols = 1024, kWaveRows = 64, kWaveThreads = GF2K_ELIM_BATCH_WAVE_THREADS;

inline long long words_of(long long bits) { return (bits + 63) >> 6; }

// a stack of matrices of m rows that the kernels can address; 0 or -1 (gf2_last_error is set)
int check_stack(const char *fn, const char *name, gf2_dmat const *M, int m) {
  const std::string n(name);
  GF2_RC(gf2_refuse_null(fn, n, M));
  if (m < 1 || m > kMaxRows) return gf2_bad_arg(fn, "matrices of " + std::to_string(m) + " rows are outside the limits (1 .. 512 rows)");
  if (M->ncols < 1 || M->ncols > kMaxCols)
    return gf2_bad_arg(fn, n + " has " + std::to_string(M->ncols) +
                               " columns: outside the limits (1 .. 1024 columns; gf2_echelonize_dev has none)");
  if (M->nrows < 0) return gf2_bad_arg(fn, n + " has a negative row count");
  if (M->nrows % m) return gf2_bad_arg(fn, n + ".nrows is not a multiple of the matrices' row count");
  if (M->nrows == 0) return 0;
  GF2_RC(gf2_refuse_null(fn, n + ".data", M->data));
  if (M->ld < words_of(M->ncols)) return gf2_bad_arg(fn, n + ".ld is smaller than the row width");
  return gf2_refuse_misaligned(fn, n + ".data", M->data, 8);
}

}  // namespace

// The only place that decides which kernel a shape runs on (gf2k_elim_batch asks here).  LDS kernel: the rows at an odd stride, the
// pivot row, 16 ints of candidates and m ints of pivot columns -- the kernel carves the same sum.
extern "C" int gf2_elim_batch_plan(int m, int ncols, int inverse, long long out[4]) {
  if (out) out[0] = out[1] = out[2] = out[3] = 0;
  if (m < 1 || m > kMaxRows || ncols < 1 || ncols > kMaxCols || (inverse && ncols != m)) return -1;
  const int aw = (int)words_of(ncols), held = inverse ? 2 * aw : aw;
  int variant;
  long long plan[4];
  if (m <= kWaveRows) {
    int w = 1, lg = 0;
    while (w < held) w <<= 1, ++lg;  // 1, 2, 4, 8, 16 words: the ids GF2K_ELIM_BATCH_WAVE1 .. WAVE16 are consecutive
    variant = inverse ? GF2K_ELIM_BATCH_WAVE_INV : GF2K_ELIM_BATCH_WAVE1 + lg;
    plan[0] = kWaveThreads;
    plan[1] = kWaveThreads / 64;
    plan[2] = 0;
    plan[3] = w;
  } else {
    const long long stride = held | 1;
    variant = inverse ? GF2K_ELIM_BATCH_LDS_INV : GF2K_ELIM_BATCH_LDS;
    plan[0] = (m + 63) / 64 * 64;
    plan[1] = 1;
    plan[2] = ((long long)m * stride + stride) * 8 + (16 + m) * 4;
    plan[3] = held;
  }
  if (out)
    for (int i = 0; i < 4; ++i) out[i] = plan[i];
  return variant;
}

extern "C" int gf2_echelonize_batch_dev(gf2_dmat *A, int m, int full, int ncols_limit, int *ranks, int *pivot_cols, void *stream) {
  static const char fn[] = "gf2_echelonize_batch_dev";
  if (int rc = check_stack(fn, "A", A, m)) return rc;
  if (ncols_limit < 0) return gf2_bad_arg(fn, "ncols_limit is negative");
  if (A->nrows == 0) return 0;
  GF2_RC(gf2_require_device_for(fn));
  const int limit = (ncols_limit > 0 && ncols_limit < A->ncols) ? ncols_limit : A->ncols;
  return gf2_hip_rc(gf2k_elim_batch(A->data, A->ld, A->data, A->ld, m, A->ncols, limit, full ? 1 : 0, 0, A->nrows / m, ranks, pivot_cols,
                                    nullptr, static_cast<hipStream_t>(stream)), fn);
}

extern "C" int gf2_inverse_batch_dev(gf2_dmat *Ainv, gf2_dmat const *A, int n, int *singular, void *stream) {
  static const char fn[] = "gf2_inverse_batch_dev";
  if (int rc = check_stack(fn, "A", A, n)) return rc;
  if (A->ncols != n) return gf2_bad_arg(fn, "the blocks of A must be n x n (A.ncols != n)");
  GF2_RC(gf2_refuse_null(fn, "Ainv", Ainv));
  if (Ainv->nrows != A->nrows || Ainv->ncols != A->ncols) return gf2_bad_arg(fn, "Ainv must have the shape of A");
  if (int rc = check_stack(fn, "Ainv", Ainv, n)) return rc;
  if (A->nrows == 0) return 0;
  if (gf2_mat_ranges_meet(A, Ainv)) return gf2_bad_arg(fn, "the address ranges of A and Ainv overlap");
  GF2_RC(gf2_require_device_for(fn));
  return gf2_hip_rc(gf2k_elim_batch(A->data, A->ld, Ainv->data, Ainv->ld, n, n, n, 1, 1, A->nrows / n, nullptr, nullptr, singular,
                                    static_cast<hipStream_t>(stream)), fn);
}
