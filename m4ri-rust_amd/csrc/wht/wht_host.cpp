// wht_host.cpp -- gf2_lpn_tally_dev, gf2_wht_dev, gf2_lpn_errors_dev, gf2_min_weight_dev and gf2_wht_plan (include/m4ri_hip_wht.h;
// kernels: gf2_wht.hip).  Every argument is checked before a device is required and before the first HIP
// call, so a bad call fails the same way with and without a device; the aliasing check comes last.  The entries only enqueue on the
// caller's stream: no host synchronisation, no hipMalloc (the partial minima come from the stream's scratch arena and are written
// before they are read; the errors are computed inside their own array).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_wht.h"
#include "../dev_args.h"
#include "gf2_wht.h"
#include "wht_plan.h"

namespace {

int check_k(const char *fn, int k) {
  if (k < 0 || k > kWhtMaxK) return gf2_bad_arg(fn, "k = " + std::to_string(k) + " is outside 0 <= k <= " + std::to_string(kWhtMaxK));
  return 0;
}

// an array of 2^k ints; align16: the transform runs over it
int check_array(const char *fn, const char *name, const void *p, int k, bool align16) {
  const std::string n(name);
  GF2_RC(gf2_check_ptr(fn, n, p, 4));
  if (align16 && k >= 2 && (reinterpret_cast<uintptr_t>(p) & 15))
    return gf2_bad_arg(fn, n + " is not 16-byte aligned (the transform of 4 or more elements moves 16 bytes per access)");
  return 0;
}

// the checks that the tally and the errors share; min_label: the lowest label column allowed (-1 or 0)
int check_tally(const char *fn, gf2_dmat const *P, int c0, int k, int label_col, int min_label, const char *name, const void *out,
                bool align16) {
  if (gf2_check_mat(fn, "P", P)) return -1;
  GF2_RC(check_k(fn, k));
  if (c0 < 0 || (long long)c0 + k > P->ncols)
    return gf2_bad_arg(fn, "the columns [c0, c0 + k) = [" + std::to_string(c0) + ", " + std::to_string((long long)c0 + k) +
                               ") are outside P (" + std::to_string(P->ncols) + " columns)");
  if (label_col < min_label || label_col >= P->ncols)
    return gf2_bad_arg(fn, "label_col = " + std::to_string(label_col) + " is outside P (" + std::to_string(P->ncols) + " columns" +
                               (min_label < 0 ? "; -1: no label)" : "; a label is required)"));
  GF2_RC(check_array(fn, name, out, k, align16));
  if (gf2_range_meets_mat(out, 4ll << k, P))
    return gf2_bad_arg(fn, std::string(name) + " and P overlap: the address range of " + name + " may not meet P's");
  return 0;
}

int enqueue_tally(const char *fn, gf2_dmat const *P, int c0, int k, int label_col, int *f, hipStream_t s) {
  GF2_RC(gf2_hip_rc(hipMemsetAsync(f, 0, (size_t)4 << k, s), fn));  // the workgroups add into it behind this, on the same stream
  if (P->nrows == 0) return 0;
  return gf2_hip_rc(gf2k_wht_tally(P->data, P->ld, P->nrows, c0, k, label_col, reinterpret_cast<unsigned *>(f), s), fn);
}

}  // namespace

extern "C" int gf2_lpn_tally_dev(gf2_dmat const *P, int c0, int k, int label_col, int *f, void *stream) {
  static const char fn[] = "gf2_lpn_tally_dev";
  GF2_RC(check_tally(fn, P, c0, k, label_col, -1, "f", f, false));
  GF2_RC(gf2_require_device());
  return enqueue_tally(fn, P, c0, k, label_col, f, static_cast<hipStream_t>(stream));
}

extern "C" int gf2_wht_dev(int *f, int k, void *stream) {
  static const char fn[] = "gf2_wht_dev";
  GF2_RC(check_k(fn, k));
  GF2_RC(check_array(fn, "f", f, k, true));
  if (k == 0) return 0;  // the identity
  GF2_RC(gf2_require_device());
  const hipError_t e = gf2k_wht_transform(reinterpret_cast<unsigned *>(f), k, 0, 0u, static_cast<hipStream_t>(stream));
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_lpn_errors_dev(gf2_dmat const *P, int c0, int k, int label_col, int *errors, void *stream) {
  static const char fn[] = "gf2_lpn_errors_dev";
  GF2_RC(check_tally(fn, P, c0, k, label_col, 0, "errors", errors, true));
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P->nrows == 0) return gf2_hip_rc(hipMemsetAsync(errors, 0, (size_t)4 << k, s), fn);  // nobody is wrong about no sample
  GF2_RC(enqueue_tally(fn, P, c0, k, label_col, errors, s));
  // the last pass stores (N - F) / 2; with k == 0 that is all the transform does
  const hipError_t e = gf2k_wht_transform(reinterpret_cast<unsigned *>(errors), k, 1, (unsigned)P->nrows, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_min_weight_dev(const int *w, int n, int *idx, int *val, void *stream) {
  static const char fn[] = "gf2_min_weight_dev";
  if (n < 1) return gf2_bad_arg(fn, "n = " + std::to_string(n) + " is below 1");
  GF2_RC(gf2_refuse_null(fn, "w", w));
  GF2_RC(gf2_refuse_null(fn, "idx", idx));
  GF2_RC(gf2_refuse_null(fn, "val", val));
  GF2_RC(gf2_refuse_misaligned(fn, "w", w, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "idx", idx, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "val", val, 4));
  if (gf2_ranges_meet(idx, 4, w, 4ll * n)) return gf2_bad_arg(fn, "idx and w overlap: idx may not lie inside w");
  if (gf2_ranges_meet(val, 4, w, 4ll * n)) return gf2_bad_arg(fn, "val and w overlap: val may not lie inside w");
  if (gf2_ranges_meet(idx, 4, val, 4)) return gf2_bad_arg(fn, "idx and val overlap");
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *partial = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)wht_min_scratch(n), &partial, GF2_SLOT_WHT_MIN_PARTIALS));
  const hipError_t e = gf2k_wht_min(w, n, idx, val, static_cast<int *>(partial), s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_wht_plan(int k, long long out[12]) {
  const WhtPlan p = wht_plan(k);
  if (p.passes < 0) return -1;
  if (out) {
    for (int i = 0; i < 8; ++i) out[i] = p.first[i];
    out[8] = kWhtThreads;
    out[9] = kWhtLdsBytes;
    out[10] = wht_tally_variant(k);
    out[11] = wht_min_scratch(1ll << k);
  }
  return p.passes;
}
