// unique_host.cpp -- gf2_sort_rows_dev, gf2_unique_rows_dev and gf2_sort_rows_plan (include/m4ri_hip_unique.h; kernels: gf2_unique.hip,
// the passes of lf2/gf2_lf2.hip and the selection of weight/gf2_weight.hip).  Every argument is checked before
// a device is required and before the first HIP call, so a bad call fails the same way with and without a device; the aliasing check
// comes last.  The entries only enqueue on the caller's stream: no host synchronisation, no hipMalloc (pair buffers, digit counts, run
// carries, the sorted order, heads, flags and block counts come from the stream's scratch arena and are written before they are read).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_unique.h"
#include "../dev_args.h"
#include "../lf2/gf2_lf2.h"
#include "../weight/gf2_weight.h"
#include "gf2_unique.h"
#include "unique_plan.h"

namespace {

// the range [c0, c1) of a call, in a matrix of ncols columns
int check_range(const char *fn, int ncols, int c0, int c1) {
  if (c0 < 0 || c0 > c1 || c1 > ncols)
    return gf2_bad_arg(fn, "the columns [c0, c1) = [" + std::to_string(c0) + ", " + std::to_string(c1) + ") are outside 0 <= c0 <= c1 <= " +
                               std::to_string(ncols) + " columns");
  return 0;
}

// order <- the rows of P ascending by (value, row): the iota for an empty range, else window after window, least significant first;
// the pairs go from one buffer to the other and the very last pass writes order.  work: unique_plan(...).work_bytes.  P->nrows > 0;
// the caller holds gf2_enqueue_mu
int enqueue_sort(const char *fn, gf2_dmat const *P, int c0, int c1, const UniquePlan &plan, void *work, int *order, hipStream_t s) {
  if (plan.windows == 0) return gf2_hip_rc(gf2k_lf2_iota(P->nrows, order, nullptr, s), fn);
  const Lf2SortWork w = lf2_sort_work(work, lf2_plan(P->nrows, 0, kUniqueWindowBits));
  int cur = 0;  // the buffer that holds the current order
  for (int win = 0; win < plan.windows; ++win) {
    const int bits = unique_window_bits(c0, c1, win), passes = lf2_plan(P->nrows, 0, bits).passes;
    GF2_RC(gf2_hip_rc(gf2k_unique_rekey(P->data, P->ld, unique_window_c0(c0, win), bits, P->nrows, win == 0, w.pairs[cur], s), fn));
    for (int pass = 0; pass < passes; ++pass, cur ^= 1) {
      const bool last = win == plan.windows - 1 && pass == passes - 1;
      const hipError_t e = gf2k_lf2_sort_pass(nullptr, 0, 0, bits, w.pairs[cur], P->nrows, pass, w.counts, w.parts,
                                              last ? nullptr : w.pairs[cur ^ 1], last ? order : nullptr, nullptr, s);
      GF2_RC(gf2_hip_rc(e, fn));
    }
  }
  return 0;
}

}  // namespace

extern "C" int gf2_sort_rows_dev(gf2_dmat const *P, int c0, int c1, int *order, int *head, void *stream) {
  static const char fn[] = "gf2_sort_rows_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  GF2_RC(check_range(fn, P->ncols, c0, c1));
  GF2_RC(gf2_check_ptr(fn, "order", order, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "head", head, 4));
  // aliasing, last
  const Gf2FlatArray arrays[2] = {{"order", order, 4ll * P->nrows}, {"head", head, 4ll * P->nrows}};
  const Gf2NamedMat mat = {"P", P};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 2, &mat, 1));
  GF2_RC(gf2_require_device_for(fn));
  if (P->nrows == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const UniquePlan plan = unique_plan(P->nrows, P->ncols, c0, c1);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.sort_scratch, &scratch, GF2_SLOT_UNIQUE));
  const UniqueWork w = unique_work(scratch, plan, P->nrows);
  GF2_RC(enqueue_sort(fn, P, c0, c1, plan, w.work, order, s));
  if (!head) return 0;
  return gf2_hip_rc(gf2k_unique_heads(P->data, P->ld, P->nrows, c0, c1, order, head, w.carry, s), fn);
}

extern "C" int gf2_unique_rows_dev(gf2_dmat const *P, int c0, int c1, int *keep, int cap, int *count, int *rep, void *stream) {
  static const char fn[] = "gf2_unique_rows_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  GF2_RC(check_range(fn, P->ncols, c0, c1));
  GF2_RC(gf2_refuse_misaligned(fn, "keep", keep, 4));
  if (cap < 0) return gf2_bad_arg(fn, "cap = " + std::to_string(cap) + " is negative");
  if (cap > 0) GF2_RC(gf2_refuse_null(fn, "keep", keep));
  GF2_RC(gf2_check_ptr(fn, "count", count, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "rep", rep, 4));
  // aliasing, last
  const Gf2FlatArray arrays[3] = {{"keep", keep, 4ll * cap}, {"count", count, 4}, {"rep", rep, 4ll * P->nrows}};
  const Gf2NamedMat mat = {"P", P};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 3, &mat, 1));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P->nrows == 0) return gf2_hip_rc(hipMemsetAsync(count, 0, 4, s), fn);
  const UniquePlan plan = unique_plan(P->nrows, P->ncols, c0, c1);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.unique_scratch, &scratch, GF2_SLOT_UNIQUE));
  const UniqueWork w = unique_work(scratch, plan, P->nrows);
  GF2_RC(enqueue_sort(fn, P, c0, c1, plan, w.work, w.order, s));
  // head and flags take the place of the first pair buffer: the sort is enqueued, and nothing behind it reads a pair
  GF2_RC(gf2_hip_rc(gf2k_unique_heads(P->data, P->ld, P->nrows, c0, c1, w.order, w.head, w.carry, s), fn));
  GF2_RC(gf2_hip_rc(gf2k_unique_rep(w.order, w.head, P->nrows, rep, w.flags, s), fn));
  return gf2_hip_rc(gf2k_weight_select(w.flags, P->nrows, 1, 1, keep, cap, count, w.blocks, s), fn);
}

extern "C" int gf2_sort_rows_plan(int nrows, int ncols, int c0, int c1, long long out[8]) {
  const UniquePlan p = unique_plan(nrows, ncols, c0, c1);
  if (p.windows < 0) return -1;
  if (out) {
    out[0] = p.windows;
    out[1] = kUniqueWindowBits;
    out[2] = p.passes;
    out[3] = p.sort_launches;
    out[4] = p.unique_launches;
    out[5] = p.sort_scratch;
    out[6] = p.unique_scratch;
    out[7] = kUniqueRunRows;
  }
  return p.passes;
}
