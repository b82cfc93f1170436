// bkw_host.cpp -- gf2_class_first_dev, gf2_lf1_reduce_dev and gf2_lf1_plan (include/m4ri_hip_bkw.h; kernels: gf2_bkw.hip; DESIGN.md
// section 7.11).  Every argument is checked before a device is required and before the first HIP call, so a bad call fails the same
// way with and without a device; the aliasing check comes last.  The entries only enqueue on the caller's stream: no host
// synchronisation, no hipMalloc (the block counts of the compaction come from the stream's scratch arena and are written before they
// are read; the table of class firsts is the caller's).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_bkw.h"
#include "../dev_args.h"
#include "bkw_plan.h"
#include "gf2_bkw.h"

namespace {

// first <- all-ones bytes, then the minima; behind this the table is final on `s`
int enqueue_first(const char *fn, gf2_dmat const *P, int c0, int b, int *first, hipStream_t s) {
  GF2_RC(gf2_hip_rc(hipMemsetAsync(first, 0xFF, (size_t)4 << b, s), fn));  // the workgroups lower it behind this, on the same stream
  if (P->nrows == 0) return 0;
  return gf2_hip_rc(gf2k_lf1_first(P->data, P->ld, P->nrows, c0, b, first, -1, s), fn);
}

}  // namespace

extern "C" int gf2_class_first_dev(gf2_dmat const *P, int c0, int b, int *first, void *stream) {
  static const char fn[] = "gf2_class_first_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  GF2_RC(gf2_check_key_window(fn, "P", P->ncols, c0, b, kLf1MaxB));
  GF2_RC(gf2_check_ptr(fn, "first", first, 4));
  const Gf2FlatArray f = {"first", first, 4ll << b};
  const Gf2NamedMat mat = {"P", P};
  GF2_RC(gf2_refuse_array_overlaps(fn, &f, 1, &mat, 1));
  GF2_RC(gf2_require_device_for(fn));
  return enqueue_first(fn, P, c0, b, first, static_cast<hipStream_t>(stream));
}

extern "C" int gf2_lf1_reduce_dev(gf2_dmat *D, gf2_dmat const *P, int c0, int b, int flags, int *first, int *count, int *src, void *stream) {
  static const char fn[] = "gf2_lf1_reduce_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  if (gf2_check_mat(fn, "D", D)) return -1;
  if (D->nrows > 0) GF2_RC(gf2_refuse_null(fn, "D.data", D->data));  // also where a row has no word
  GF2_RC(gf2_check_key_window(fn, "P", P->ncols, c0, b, kLf1MaxB));
  if (flags & ~GF2_LF1_KEEP_ZERO) return gf2_bad_arg(fn, "flags = " + std::to_string(flags) + " has bits other than GF2_LF1_KEEP_ZERO");
  if (D->ncols != P->ncols)
    return gf2_bad_arg(fn, "D has " + std::to_string(D->ncols) + " columns, P " + std::to_string(P->ncols) + ": D->ncols must equal P->ncols");
  GF2_RC(gf2_check_ptr(fn, "first", first, 4));
  GF2_RC(gf2_check_ptr(fn, "count", count, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "src", src, 4));
  // aliasing, last
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "P", P));
  const Gf2FlatArray arrays[3] = {{"first", first, 4ll << b}, {"count", count, 4}, {"src", src, 4ll * D->nrows}};
  const Gf2NamedMat mats[2] = {{"P", P}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 3, mats, 2));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  GF2_RC(enqueue_first(fn, P, c0, b, first, s));
  if (P->nrows == 0) return gf2_hip_rc(hipMemsetAsync(count, 0, 4, s), fn);
  const Lf1Plan plan = lf1_plan(P->nrows, P->ncols, b);
  const int keep_zero = flags & GF2_LF1_KEEP_ZERO ? 1 : 0;
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &scratch, GF2_SLOT_BKW_BLOCK_COUNTS));
  int *counts = static_cast<int *>(scratch);
  GF2_RC(gf2_hip_rc(gf2k_lf1_count(P->data, P->ld, P->nrows, P->ncols, c0, b, keep_zero, first, counts, s), fn));
  GF2_RC(gf2_hip_rc(gf2k_lf1_scan(counts, plan.blocks, count, s), fn));
  if (D->nrows == 0) return 0;  // a count-only call
  const hipError_t e = gf2k_lf1_scatter(P->data, P->ld, P->nrows, P->ncols, c0, b, keep_zero, first, counts, D->data, D->ld, D->nrows, src, -1, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_lf1_plan(int nrows, int ncols, int b, long long out[5]) {
  const Lf1Plan p = lf1_plan(nrows, ncols, b);
  if (p.variant < 0) return -1;
  if (out) {
    out[0] = kLf1FirstThreads;
    out[1] = p.variant == 0 ? 4ll << b : 0;
    out[2] = p.rows;
    out[3] = p.lanes;
    out[4] = p.scratch;
  }
  return p.variant;
}
