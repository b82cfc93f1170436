// lf2_host.cpp -- gf2_class_sort_dev, gf2_lf2_reduce_dev and gf2_lf2_plan (include/m4ri_hip_lf2.h; kernels: gf2_lf2.hip; DESIGN.md
// section 7.13).  Every argument is checked before a device is required and before the first HIP call, so a bad call fails the same
// way with and without a device; the aliasing check comes last.  The entries only enqueue on the caller's stream: no host
// synchronisation, no hipMalloc (pair buffers, digit counts, the sorted order of a round and its run sums come from the stream's
// scratch arena and are written before they are read).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_lf2.h"
#include "../dev_args.h"
#include "gf2_lf2.h"
#include "lf2_plan.h"

int gf2_enqueue_class_sort(const char *fn, gf2_dmat const *M, int c0, int b, void *work, int *order, int *skeys, hipStream_t s) {
  const Lf2Plan plan = lf2_plan(M->nrows, M->ncols, b);
  if (plan.passes == 0) return gf2_hip_rc(gf2k_lf2_iota(M->nrows, order, skeys, s), fn);
  const Lf2SortWork w = lf2_sort_work(work, plan);
  for (int pass = 0; pass < plan.passes; ++pass) {
    const bool first = pass == 0, last = pass == plan.passes - 1;
    const hipError_t e = gf2k_lf2_sort_pass(first ? M->data : nullptr, M->ld, c0, b, first ? nullptr : w.pairs[(pass - 1) & 1], M->nrows, pass,
                                            w.counts, w.parts, last ? nullptr : w.pairs[pass & 1], last ? order : nullptr,
                                            last ? skeys : nullptr, s);
    GF2_RC(gf2_hip_rc(e, fn));
  }
  return 0;
}

namespace {

// the sort in a work space of its own from the stream's arena (none for b == 0: the iota needs none).  The caller holds gf2_enqueue_mu
int sort_in_arena(const char *fn, gf2_dmat const *P, int c0, int b, int *order, int *skeys, hipStream_t s) {
  void *work = nullptr;
  const Lf2Plan plan = lf2_plan(P->nrows, P->ncols, b);
  if (plan.passes > 0) GF2_RC(gf2_stream_scratch(s, (size_t)plan.sort_scratch, &work, GF2_SLOT_LF2_SORT));
  return gf2_enqueue_class_sort(fn, P, c0, b, work, order, skeys, s);
}

}  // namespace

extern "C" int gf2_class_sort_dev(gf2_dmat const *P, int c0, int b, int *order, int *skeys, void *stream) {
  static const char fn[] = "gf2_class_sort_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  GF2_RC(gf2_check_key_window(fn, "P", P->ncols, c0, b, kLf2MaxB));
  GF2_RC(gf2_check_ptr(fn, "order", order, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "skeys", skeys, 4));
  // aliasing, last
  const Gf2FlatArray arrays[2] = {{"order", order, 4ll * P->nrows}, {"skeys", skeys, 4ll * P->nrows}};
  const Gf2NamedMat mat = {"P", P};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 2, &mat, 1));
  GF2_RC(gf2_require_device_for(fn));
  if (P->nrows == 0) return 0;
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  return sort_in_arena(fn, P, c0, b, order, skeys, static_cast<hipStream_t>(stream));
}

extern "C" int gf2_lf2_reduce_dev(gf2_dmat *D, gf2_dmat const *P, int c0, int b, long long *count, int *lo, int *hi, void *stream) {
  static const char fn[] = "gf2_lf2_reduce_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  if (gf2_check_mat(fn, "D", D)) return -1;
  if (D->nrows > 0) GF2_RC(gf2_refuse_null(fn, "D.data", D->data));  // also where a row has no word
  GF2_RC(gf2_check_key_window(fn, "P", P->ncols, c0, b, kLf2MaxB));
  if (D->ncols != P->ncols)
    return gf2_bad_arg(fn, "D has " + std::to_string(D->ncols) + " columns, P " + std::to_string(P->ncols) + ": D->ncols must equal P->ncols");
  GF2_RC(gf2_check_ptr(fn, "count", count, 8));
  GF2_RC(gf2_refuse_misaligned(fn, "lo", lo, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "hi", hi, 4));
  // aliasing, last
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "P", P));
  const Gf2FlatArray arrays[3] = {{"count", count, 8}, {"lo", lo, 4ll * D->nrows}, {"hi", hi, 4ll * D->nrows}};
  const Gf2NamedMat mats[2] = {{"P", P}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 3, mats, 2));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P->nrows == 0) return gf2_hip_rc(hipMemsetAsync(count, 0, 8, s), fn);
  const Lf2Plan plan = lf2_plan(P->nrows, P->ncols, b);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.pair_scratch, &scratch, GF2_SLOT_LF2_PAIRS));
  char *base = static_cast<char *>(scratch);
  int *order = reinterpret_cast<int *>(base), *skeys = reinterpret_cast<int *>(base + plan.order_bytes);
  long long *sums = reinterpret_cast<long long *>(base + 2 * plan.order_bytes);
  GF2_RC(sort_in_arena(fn, P, c0, b, order, skeys, s));
  GF2_RC(gf2_hip_rc(gf2k_lf2_pair_count(skeys, P->nrows, sums, count, s), fn));
  if (D->nrows == 0) return 0;  // a count-only call
  const hipError_t e = gf2k_lf2_pair_scatter(P->data, P->ld, P->nrows, P->ncols, order, skeys, sums, D->data, D->ld, D->nrows, lo, hi, -1, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_lf2_plan(int nrows, int ncols, int b, long long out[8]) {
  const Lf2Plan p = lf2_plan(nrows, ncols, b);
  if (p.passes < 0) return -1;
  if (out) {
    out[0] = kLf2DigitBits;
    out[1] = kLf2Threads;
    out[2] = kLf2SortLds;
    out[3] = kLf2TileRows;
    out[4] = kLf2RunRows;
    out[5] = p.lanes;
    out[6] = p.sort_scratch;
    out[7] = p.pair_scratch + p.sort_scratch;
  }
  return p.passes;
}
