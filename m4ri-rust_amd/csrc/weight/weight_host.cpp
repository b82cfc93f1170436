// weight_host.cpp -- gf2_row_weights_dev, gf2_col_weights_dev, gf2_count_ones_dev, gf2_select_weights_dev and gf2_weights_plan
// (include/m4ri_hip_weight.h; kernels: gf2_weight.hip).  Every argument is checked before a device is required
// and before the first HIP call, so a bad call fails the same way with and without a device, and an output of length 0 returns without
// one.  The entries only enqueue on the caller's stream: no host synchronisation, no hipMalloc (the partial sums of the column
// weights and the block counts of the selection come from the stream's scratch arena and are written before they are read).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_weight.h"
#include "../dev_args.h"
#include "gf2_weight.h"
#include "weight_plan.h"

namespace {

// 0: go ahead; 1: nothing to do; -1: refused (gf2_last_error is set).  `out` holds `count` elements of `size` bytes
int check_call(const char *fn, gf2_dmat const *A, const char *name, const void *out, long long count, int size) {
  if (gf2_check_mat(fn, "A", A)) return -1;
  if (count == 0) return 1;
  const std::string n(name);
  GF2_RC(gf2_check_ptr(fn, n, out, size));
  if (gf2_range_meets_mat(out, count * size, A))
    return gf2_bad_arg(fn, n + " and A overlap: the address range of " + n + " may not meet A's");
  return 0;
}

int clear_async(const char *fn, void *p, size_t bytes, hipStream_t s) { return gf2_hip_rc(hipMemsetAsync(p, 0, bytes, s), fn); }

}  // namespace

extern "C" int gf2_row_weights_dev(gf2_dmat const *A, int *weights, void *stream) {
  static const char fn[] = "gf2_row_weights_dev";
  if (int rc = check_call(fn, A, "weights", weights, A ? A->nrows : 0, 4)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->ncols == 0) return clear_async(fn, weights, 4 * (size_t)A->nrows, s);
  const hipError_t e = gf2k_weight_rows(A->data, A->ld, A->nrows, A->ncols, weights, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_col_weights_dev(gf2_dmat const *A, int *weights, void *stream) {
  static const char fn[] = "gf2_col_weights_dev";
  if (int rc = check_call(fn, A, "weights", weights, A ? A->ncols : 0, 4)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0) return clear_async(fn, weights, 4 * (size_t)A->ncols, s);
  const WeightColsPlan plan = weight_cols_plan(A->nrows, A->ncols);
  if (plan.scratch == 0) {
    const hipError_t e = gf2k_weight_cols(A->data, A->ld, A->nrows, A->ncols, weights, nullptr, s);
    return gf2_hip_rc(e, fn);
  }
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *partial = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &partial, GF2_SLOT_WEIGHT_COL_PARTIALS));
  const hipError_t e = gf2k_weight_cols(A->data, A->ld, A->nrows, A->ncols, weights, static_cast<int *>(partial), s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_count_ones_dev(gf2_dmat const *A, unsigned long long *total, void *stream) {
  static const char fn[] = "gf2_count_ones_dev";
  if (int rc = check_call(fn, A, "total", total, 1, 8)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  GF2_RC(clear_async(fn, total, 8, s));  // the workgroups add into it behind this, on the same stream
  const hipError_t e = gf2k_weight_total(A->data, A->ld, A->nrows, A->ncols, total, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_select_weights_dev(const int *weights, int n, int lo, int hi, int *idx, int cap, int *count, void *stream) {
  static const char fn[] = "gf2_select_weights_dev";
  if (n < 0) return gf2_bad_arg(fn, "n is negative");
  if (cap < 0) return gf2_bad_arg(fn, "cap is negative");
  if (n > 0) GF2_RC(gf2_refuse_null(fn, "weights", weights));
  GF2_RC(gf2_refuse_null(fn, "count", count));
  if (cap > 0) GF2_RC(gf2_refuse_null(fn, "idx", idx));
  GF2_RC(gf2_refuse_misaligned(fn, "weights", weights, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "idx", idx, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "count", count, 4));
  if (n == 0 && cap == 0) return 0;
  if (idx && gf2_ranges_meet(idx, 4ll * cap, weights, 4ll * n))
    return gf2_bad_arg(fn, "idx and weights overlap: the address range of idx may not meet that of weights");
  if (gf2_ranges_meet(count, 4, weights, 4ll * n)) return gf2_bad_arg(fn, "count and weights overlap: count may not lie inside weights");
  if (idx && gf2_ranges_meet(count, 4, idx, 4ll * cap)) return gf2_bad_arg(fn, "count and idx overlap: count may not lie inside idx");
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return clear_async(fn, count, 4, s);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  const long long nblk = ((long long)n + kWeightSelectBlock - 1) / kWeightSelectBlock;
  void *counts = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)(4 * nblk), &counts, GF2_SLOT_WEIGHT_SELECT_COUNTS));
  const hipError_t e = gf2k_weight_select(weights, n, lo, hi, idx, cap, count, static_cast<int *>(counts), s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_weights_plan(int what, int nrows, int ncols, long long out[4]) {
  long long o[4] = {0, 0, 0, 0};
  int variant = -1;
  if (what == 0) {
    const WeightRowsPlan p = weight_rows_plan(nrows, ncols);
    variant = p.variant;
    o[0] = kWeightThreads;
    o[1] = p.rows;
  } else if (what == 1) {
    const WeightColsPlan p = weight_cols_plan(nrows, ncols);
    variant = p.variant;
    o[0] = kWeightColThreads;
    o[1] = p.wy;
    o[2] = kWeightFlushRows;
    o[3] = p.scratch;
  } else if (what == 2) {
    const WeightTotalPlan p = weight_total_plan(nrows, ncols);
    variant = p.variant;
    o[0] = kWeightThreads;
    o[1] = p.rows;
  }
  if (variant < 0) return -1;
  if (out)
    for (int i = 0; i < 4; ++i) out[i] = o[i];
  return variant;
}
