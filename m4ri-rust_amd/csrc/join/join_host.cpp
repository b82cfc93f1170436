// join_host.cpp -- gf2_join_dev and gf2_join_plan (include/m4ri_hip_join.h; kernels: gf2_join.hip), and
// gf2_join_select_dev and gf2_join_select_plan (include/m4ri_hip_join_select.h; kernels: gf2_join_select.inc; section 7.15.1).  Every
// argument is checked before a device is required and before the first HIP call, so a bad call fails the same way with and without a
// device; the aliasing check comes last.  The entry only enqueues on the caller's stream: no host synchronisation, no hipMalloc (the
// sort's work space, the sorted orders and keys of A and B and the run sums come from the stream's scratch arena and are written
// before they are read).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_join.h"
#include "../../../include/m4ri_hip_join_select.h"
#include "../dev_args.h"
#include "../lf2/gf2_lf2.h"
#include "gf2_join.h"
#include "join_plan.h"

extern "C" int gf2_join_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int c0, int b, long long *count, int *ia, int *ib, int *wt,
                            int wc0, int wc1, void *stream) {
  static const char fn[] = "gf2_join_dev";
  if (gf2_check_mat(fn, "A", A)) return -1;
  if (gf2_check_mat(fn, "B", B)) return -1;
  if (gf2_check_mat(fn, "D", D)) return -1;
  if (D->nrows > 0) GF2_RC(gf2_refuse_null(fn, "D.data", D->data));  // also where a row has no word
  GF2_RC(gf2_check_key_bits(fn, b, kJoinMaxB));
  GF2_RC(gf2_check_equal_ncols(fn, A, B, D));
  GF2_RC(gf2_check_key_columns(fn, "A and B", A->ncols, c0, b));
  GF2_RC(gf2_check_ptr(fn, "count", count, 8));
  GF2_RC(gf2_refuse_misaligned(fn, "ia", ia, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "ib", ib, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "wt", wt, 4));
  GF2_RC(gf2_check_weight_range(fn, A->ncols, wc0, wc1));
  // aliasing, last.  A and B are only read: they may overlap or be one view
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "A", A));
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "B", B));
  const Gf2FlatArray arrays[4] = {{"count", count, 8}, {"ia", ia, 4ll * D->nrows}, {"ib", ib, 4ll * D->nrows}, {"wt", wt, 4ll * D->nrows}};
  const Gf2NamedMat mats[3] = {{"A", A}, {"B", B}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 4, mats, 3));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0 || B->nrows == 0) return gf2_hip_rc(hipMemsetAsync(count, 0, 8, s), fn);
  const JoinPlan plan = join_plan(A->nrows, B->nrows, A->ncols, b);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &scratch, GF2_SLOT_JOIN));
  char *base = static_cast<char *>(scratch), *at = base + plan.sort_bytes;
  int *order_a = reinterpret_cast<int *>(at), *skeys_a = reinterpret_cast<int *>(at + plan.order_a);
  at += 2 * plan.order_a;
  int *order_b = reinterpret_cast<int *>(at), *skeys_b = reinterpret_cast<int *>(at + plan.order_b);
  long long *sums = reinterpret_cast<long long *>(at + 2 * plan.order_b);
  GF2_RC(gf2_enqueue_class_sort(fn, A, c0, b, base, order_a, skeys_a, s));
  GF2_RC(gf2_enqueue_class_sort(fn, B, c0, b, base, order_b, skeys_b, s));  // behind A's sort on the stream: the work space is free again
  GF2_RC(gf2_hip_rc(gf2k_join_count(skeys_a, A->nrows, skeys_b, B->nrows, sums, count, s), fn));
  if (D->nrows == 0) return 0;  // a count-only call
  const hipError_t e = gf2k_join_scatter(A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, A->ncols, order_a, skeys_a, order_b, skeys_b, sums,
                                         D->data, D->ld, D->nrows, ia, ib, wt, wc0, wc1, -1, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_join_plan(int nrows_a, int nrows_b, int ncols, int b, long long out[8]) {
  const JoinPlan p = join_plan(nrows_a, nrows_b, ncols, b);
  if (p.passes < 0) return -1;
  if (out) {
    out[0] = kJoinThreads;
    out[1] = kJoinRunRows;
    out[2] = p.lanes;
    out[3] = kJoinSpanKeys;
    out[4] = kJoinLds;
    out[5] = p.scratch;
    out[6] = p.runs;
    out[7] = p.sort_bytes;
  }
  return p.passes;
}

// ---- the weight-filtered join (include/m4ri_hip_join_select.h; kernels: gf2_join_select.inc)

extern "C" int gf2_join_select_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int c0, int b, int wc0, int wc1, int wlo, int whi,
                                   long long *count, long long *hits, int *ia, int *ib, int *wt, void *stream) {
  static const char fn[] = "gf2_join_select_dev";
  if (gf2_check_mat(fn, "A", A)) return -1;
  if (gf2_check_mat(fn, "B", B)) return -1;
  if (gf2_check_mat(fn, "D", D, /*unstored_ok=*/true)) return -1;  // D->data null: the rows are not stored
  GF2_RC(gf2_check_key_bits(fn, b, kJoinMaxB));
  GF2_RC(gf2_check_equal_ncols(fn, A, B, D));
  GF2_RC(gf2_check_key_columns(fn, "A and B", A->ncols, c0, b));
  GF2_RC(gf2_check_ptr(fn, "count", count, 8));
  GF2_RC(gf2_check_ptr(fn, "hits", hits, 8));
  GF2_RC(gf2_refuse_misaligned(fn, "ia", ia, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "ib", ib, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "wt", wt, 4));
  GF2_RC(gf2_check_weight_range(fn, A->ncols, wc0, wc1));
  GF2_RC(gf2_check_weight_window(fn, wlo, whi));
  // aliasing, last.  A and B are only read: they may overlap or be one view.  A D without data shares no word with anything
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "A", A));
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "B", B));
  const Gf2FlatArray arrays[5] = {{"count", count, 8}, {"hits", hits, 8}, {"ia", ia, 4ll * D->nrows}, {"ib", ib, 4ll * D->nrows},
                                  {"wt", wt, 4ll * D->nrows}};
  const Gf2NamedMat mats[3] = {{"A", A}, {"B", B}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 5, mats, 3));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0 || B->nrows == 0) {
    GF2_RC(gf2_hip_rc(hipMemsetAsync(count, 0, 8, s), fn));
    return gf2_hip_rc(hipMemsetAsync(hits, 0, 8, s), fn);
  }
  const JoinSelectPlan plan = join_select_plan(A->nrows, B->nrows, A->ncols, b, wc0, wc1);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &scratch, GF2_SLOT_JOIN));
  char *base = static_cast<char *>(scratch), *at = base + plan.join.sort_bytes;
  int *order_a = reinterpret_cast<int *>(at), *skeys_a = reinterpret_cast<int *>(at + plan.join.order_a);
  at += 2 * plan.join.order_a;
  int *order_b = reinterpret_cast<int *>(at), *skeys_b = reinterpret_cast<int *>(at + plan.join.order_b);
  long long *sums = reinterpret_cast<long long *>(at + 2 * plan.join.order_b);
  long long *hsums = reinterpret_cast<long long *>(base + plan.join.scratch);  // behind everything of the join
  long long *hown = reinterpret_cast<long long *>(base + plan.join.scratch + plan.hit_bytes / 2);
  GF2_RC(gf2_enqueue_class_sort(fn, A, c0, b, base, order_a, skeys_a, s));
  GF2_RC(gf2_enqueue_class_sort(fn, B, c0, b, base, order_b, skeys_b, s));  // behind A's sort on the stream: the work space is free again
  GF2_RC(gf2_hip_rc(gf2k_join_count(skeys_a, A->nrows, skeys_b, B->nrows, sums, count, s), fn));
  GF2_RC(gf2_hip_rc(gf2k_join_weigh(A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, A->ncols, order_a, skeys_a, order_b, skeys_b, hsums,
                                    hown, hits, wc0, wc1, wlo, whi, -1, s),
                    fn));
  const bool stored = D->data != nullptr && D->ncols > 0;
  if (D->nrows == 0 || (!stored && !ia && !ib && !wt)) return 0;  // the counts only (the second: rows that are not stored, and no array)
  const hipError_t e = gf2k_join_select_scatter(A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, A->ncols, order_a, skeys_a, order_b, skeys_b,
                                                hsums, hown, stored ? D->data : nullptr, D->ld, D->nrows, ia, ib, wt, wc0, wc1, wlo, whi, -1, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_join_select_plan(int nrows_a, int nrows_b, int ncols, int b, int wc0, int wc1, long long out[8]) {
  if (wc0 < 0 || wc0 > wc1 || wc1 > ncols) return -1;
  const JoinSelectPlan p = join_select_plan(nrows_a, nrows_b, ncols, b, wc0, wc1);
  if (p.join.passes < 0) return -1;
  if (out) {
    out[0] = kJoinThreads;
    out[1] = kJoinRunRows;
    out[2] = p.weigh_lanes;
    out[3] = p.join.lanes;
    out[4] = kJoinSelectLds;
    out[5] = p.scratch;
    out[6] = p.join.runs;
    out[7] = p.round_outputs;
  }
  return p.join.passes;
}
