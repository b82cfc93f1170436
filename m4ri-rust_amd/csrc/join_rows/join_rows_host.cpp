// join_rows_host.cpp -- gf2_group_rows_dev, gf2_join_rows_dev and gf2_join_rows_plan (include/m4ri_hip_join_rows.h; kernels:
// gf2_join_rows.hip, the table of find/gf2_find.hip and the passes of lf2/gf2_lf2.hip).  Every argument is
// checked before a device is required and before the first HIP call, so a bad call fails the same way with and without a device; the
// aliasing check comes last.  The entries only enqueue on the caller's stream: no host synchronisation, no hipMalloc (the table, rep,
// the class starts, the sort's work space, the sorted order of B, idx and mult of A, the offsets and the run sums come from the
// stream's scratch arena and are written before they are read).
//
// The table is reached through gf2k_find_rows, the launcher that gf2_find_rows_dev uses: fill, build and lookup in one.  The join
// calls it twice -- A in B for idx and mult, B in B for rep -- and so builds the table of B twice; gf2_find.hip stays as it is.
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_join_rows.h"
#include "../dev_args.h"
#include "../find/gf2_find.h"
#include "../lf2/gf2_lf2.h"
#include "gf2_join_rows.h"
#include "join_rows_plan.h"

namespace {

// the range [c0, c1) of a call, in a matrix of ncols columns
int check_range(const char *fn, int ncols, int c0, int c1) {
  if (c0 < 0 || c0 > c1 || c1 > ncols)
    return gf2_bad_arg(fn, "the columns [c0, c1) = [" + std::to_string(c0) + ", " + std::to_string(c1) + ") are outside 0 <= c0 <= c1 <= " +
                               std::to_string(ncols) + " columns");
  return 0;
}

// rep <- the lowest equal row of every row of P; order <- the rows of P ascending by (rep, row): the iota for a single row, else the
// pairs of every window and its passes, least significant window first; the pairs go from one buffer to the other and the very last
// pass writes order.  P->nrows > 0; the caller holds gf2_enqueue_mu
int enqueue_group(const char *fn, gf2_dmat const *P, int c0, int c1, const JoinRowsPlan &plan, const JoinRowsWork &w, int *order,
                  hipStream_t s) {
  GF2_RC(gf2_hip_rc(gf2k_find_rows(P->data, P->ld, P->nrows, P->data, P->ld, P->nrows, c0, c1, w.table, w.rep, nullptr, nullptr, s), fn));
  if (plan.passes == 0) return gf2_hip_rc(gf2k_lf2_iota(P->nrows, order, nullptr, s), fn);
  const Lf2SortWork sw = lf2_sort_work(w.work, lf2_plan(P->nrows, 0, kJoinRowsLowBits));
  int cur = 0;  // the buffer that holds the current order
  for (int win = 0; win < plan.windows; ++win) {
    const int bits = join_rows_window_bits(plan.bits, win), passes = lf2_plan(P->nrows, 0, bits).passes;
    GF2_RC(gf2_hip_rc(gf2k_join_rows_pairs(w.rep, P->nrows, join_rows_window_shift(plan.bits, win), bits, win == 0, sw.pairs[cur], s), fn));
    for (int pass = 0; pass < passes; ++pass, cur ^= 1) {
      const bool last = win == plan.windows - 1 && pass == passes - 1;
      const hipError_t e = gf2k_lf2_sort_pass(nullptr, 0, 0, bits, sw.pairs[cur], P->nrows, pass, sw.counts, sw.parts,
                                              last ? nullptr : sw.pairs[cur ^ 1], last ? order : nullptr, nullptr, s);
      GF2_RC(gf2_hip_rc(e, fn));
    }
  }
  return 0;
}

}  // namespace

extern "C" int gf2_group_rows_dev(gf2_dmat const *P, int c0, int c1, int *order, int *head, void *stream) {
  static const char fn[] = "gf2_group_rows_dev";
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
  const JoinRowsPlan plan = join_rows_plan(0, P->nrows, P->ncols, c0, c1);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.group_scratch, &scratch, GF2_SLOT_JOIN_ROWS));
  const JoinRowsWork w = join_rows_work(scratch, plan, false);
  GF2_RC(enqueue_group(fn, P, c0, c1, plan, w, order, s));
  if (!head) return 0;
  GF2_RC(gf2_hip_rc(gf2k_join_rows_starts(order, w.rep, P->nrows, w.start, s), fn));
  return gf2_hip_rc(gf2k_join_rows_heads(order, w.rep, w.start, P->nrows, head, s), fn);
}

extern "C" int gf2_join_rows_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int c0, int c1, long long *count, int *ia, int *ib,
                                 int *wt, int wc0, int wc1, void *stream) {
  static const char fn[] = "gf2_join_rows_dev";
  if (gf2_check_mat(fn, "A", A)) return -1;
  if (gf2_check_mat(fn, "B", B)) return -1;
  if (gf2_check_mat(fn, "D", D, /*unstored_ok=*/true)) return -1;  // D->data null: the rows are not stored
  GF2_RC(gf2_check_equal_ncols(fn, A, B, D));
  GF2_RC(check_range(fn, A->ncols, c0, c1));
  GF2_RC(gf2_check_ptr(fn, "count", count, 8));
  GF2_RC(gf2_refuse_misaligned(fn, "ia", ia, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "ib", ib, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "wt", wt, 4));
  GF2_RC(gf2_check_weight_range(fn, A->ncols, wc0, wc1));
  // aliasing, last.  A and B are only read: they may overlap or be one view.  A D without data shares no word with anything
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "A", A));
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "B", B));
  const Gf2FlatArray arrays[4] = {{"count", count, 8}, {"ia", ia, 4ll * D->nrows}, {"ib", ib, 4ll * D->nrows}, {"wt", wt, 4ll * D->nrows}};
  const Gf2NamedMat mats[3] = {{"A", A}, {"B", B}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 4, mats, 3));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0 || B->nrows == 0) return gf2_hip_rc(hipMemsetAsync(count, 0, 8, s), fn);
  const JoinRowsPlan plan = join_rows_plan(A->nrows, B->nrows, A->ncols, c0, c1);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.join_scratch, &scratch, GF2_SLOT_JOIN_ROWS));
  const JoinRowsWork w = join_rows_work(scratch, plan, true);
  GF2_RC(gf2_hip_rc(gf2k_find_rows(A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, c0, c1, w.table, w.idx, w.mult, nullptr, s), fn));
  GF2_RC(gf2_hip_rc(gf2k_join_rows_count(w.mult, A->nrows, w.sums, count, s), fn));
  const bool stored = D->data != nullptr && D->ncols > 0;
  if (D->nrows == 0 || (!stored && !ia && !ib && !wt)) return 0;  // the count only (the second: rows that are not stored, and no array)
  GF2_RC(gf2_hip_rc(gf2k_join_rows_offsets(w.mult, A->nrows, w.sums, w.offs, s), fn));
  GF2_RC(enqueue_group(fn, B, c0, c1, plan, w, w.order, s));  // behind the lookup of A on the stream: the table is free again
  GF2_RC(gf2_hip_rc(gf2k_join_rows_starts(w.order, w.rep, B->nrows, w.start, s), fn));
  const hipError_t e = gf2k_join_rows_scatter(A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, A->ncols, w.idx, w.offs, w.order, w.start, count,
                                              stored ? D->data : nullptr, D->ld, D->nrows, ia, ib, wt, wc0, wc1, -1, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_join_rows_plan(int nrows_a, int nrows_b, int ncols, int c0, int c1, long long out[8]) {
  const JoinRowsPlan p = join_rows_plan(nrows_a, nrows_b, ncols, c0, c1);
  if (p.passes < 0) return -1;
  if (out) {
    out[0] = p.slots;
    out[1] = p.wave;
    out[2] = p.group_launches;
    out[3] = p.join_launches;
    out[4] = kJoinRowsRunRows;
    out[5] = kJoinRowsChunk;
    out[6] = p.group_scratch;
    out[7] = p.join_scratch;
  }
  return p.passes;
}
