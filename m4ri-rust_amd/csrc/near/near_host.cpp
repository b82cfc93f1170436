// near_host.cpp -- gf2_near_pairs_dev, gf2_nearest_dev and gf2_near_plan (include/m4ri_hip_near.h; kernels: gf2_near.hip; DESIGN.md
// section 7.17).  Every argument is checked before a device is required and before the first HIP call, so a bad call fails the same
// way with and without a device; the aliasing check comes last.  The entries only enqueue on the caller's stream: no host
// synchronisation, no hipMalloc (the cells -- hit counts or chunk minima -- come from the stream's scratch arena and are written before
// they are read).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_near.h"
#include "../dev_args.h"
#include "gf2_near.h"
#include "near_plan.h"

namespace {

// the checks that both entries share, in the order of the arguments: the pools, their widths, the range, the flags
int check_pools(const char *fn, gf2_dmat const *A, gf2_dmat const *B) {
  if (gf2_check_mat(fn, "A", A)) return -1;
  if (gf2_check_mat(fn, "B", B)) return -1;
  return 0;
}
int check_flags(const char *fn, int flags) {
  if (flags & ~(GF2_NEAR_OFF_DIAGONAL | GF2_NEAR_UPPER))
    return gf2_bad_arg(fn, "flags = " + std::to_string(flags) + " has bits other than GF2_NEAR_OFF_DIAGONAL (1) and GF2_NEAR_UPPER (2)");
  return 0;
}
NearOperands operands(gf2_dmat const *A, gf2_dmat const *B, int wc0, int wc1, int flags) {
  return {A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, A->ncols, wc0, wc1, flags};
}

}  // namespace

extern "C" int gf2_near_pairs_dev(gf2_dmat *D, gf2_dmat const *A, gf2_dmat const *B, int wc0, int wc1, int wlo, int whi, int flags,
                                  long long *hits, int *ia, int *ib, int *wt, void *stream) {
  static const char fn[] = "gf2_near_pairs_dev";
  GF2_RC(check_pools(fn, A, B));
  if (gf2_check_mat(fn, "D", D, /*unstored_ok=*/true)) return -1;  // D->data null: the rows are not stored
  GF2_RC(gf2_check_equal_ncols(fn, A, B, D));
  GF2_RC(gf2_check_ptr(fn, "hits", hits, 8));
  GF2_RC(gf2_refuse_misaligned(fn, "ia", ia, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "ib", ib, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "wt", wt, 4));
  GF2_RC(gf2_check_weight_range(fn, A->ncols, wc0, wc1));
  GF2_RC(gf2_check_weight_window(fn, wlo, whi));
  GF2_RC(check_flags(fn, flags));
  // aliasing, last.  A and B are only read: they may overlap or be one view.  A D without data shares no word with anything
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "A", A));
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "B", B));
  const Gf2FlatArray arrays[4] = {{"hits", hits, 8}, {"ia", ia, 4ll * D->nrows}, {"ib", ib, 4ll * D->nrows}, {"wt", wt, 4ll * D->nrows}};
  const Gf2NamedMat mats[3] = {{"A", A}, {"B", B}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 4, mats, 3));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0 || B->nrows == 0) return gf2_hip_rc(hipMemsetAsync(hits, 0, 8, s), fn);
  const NearPlan plan = near_plan(A->nrows, B->nrows, A->ncols, wc0, wc1);
  const NearOperands o = operands(A, B, wc0, wc1, flags);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &scratch, GF2_SLOT_NEAR));
  long long *cells = static_cast<long long *>(scratch);
  GF2_RC(gf2_hip_rc(gf2k_near_count(&o, wlo, whi, cells, hits, s), fn));
  const bool stored = D->data != nullptr && D->ncols > 0;
  if (D->nrows == 0 || (!stored && !ia && !ib && !wt)) return 0;  // the count only (the second: rows that are not stored, and no array)
  return gf2_hip_rc(gf2k_near_select(&o, wlo, whi, cells, stored ? D->data : nullptr, D->ld, D->nrows, ia, ib, wt, s), fn);
}

extern "C" int gf2_nearest_dev(gf2_dmat const *A, gf2_dmat const *B, int wc0, int wc1, int flags, int *idx, int *dist, void *stream) {
  static const char fn[] = "gf2_nearest_dev";
  GF2_RC(check_pools(fn, A, B));
  if (B->ncols != A->ncols)
    return gf2_bad_arg(fn, "A has " + std::to_string(A->ncols) + " columns, B " + std::to_string(B->ncols) + ": A->ncols and B->ncols must be equal");
  if (!idx && !dist) return gf2_bad_arg(fn, "idx and dist are both null: one of them must be given");
  GF2_RC(gf2_refuse_misaligned(fn, "idx", idx, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "dist", dist, 4));
  GF2_RC(gf2_check_weight_range(fn, A->ncols, wc0, wc1));
  GF2_RC(check_flags(fn, flags));
  // aliasing, last
  const Gf2FlatArray arrays[2] = {{"idx", idx, 4ll * A->nrows}, {"dist", dist, 4ll * A->nrows}};
  const Gf2NamedMat mats[2] = {{"A", A}, {"B", B}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 2, mats, 2));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0) return 0;
  if (B->nrows == 0) {  // no partner: -1 in every entry
    if (idx) GF2_RC(gf2_hip_rc(hipMemsetAsync(idx, 0xFF, 4ull * A->nrows, s), fn));
    if (dist) GF2_RC(gf2_hip_rc(hipMemsetAsync(dist, 0xFF, 4ull * A->nrows, s), fn));
    return 0;
  }
  const NearPlan plan = near_plan(A->nrows, B->nrows, A->ncols, wc0, wc1);
  const NearOperands o = operands(A, B, wc0, wc1, flags);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &scratch, GF2_SLOT_NEAR));
  return gf2_hip_rc(gf2k_nearest(&o, static_cast<long long *>(scratch), idx, dist, s), fn);
}

extern "C" int gf2_near_plan(int nrows_a, int nrows_b, int ncols, int wc0, int wc1, long long out[8]) {
  const NearPlan p = near_plan(nrows_a, nrows_b, ncols, wc0, wc1);
  if (p.kernel < 0) return -1;
  if (out) {
    out[0] = p.kernel;
    out[1] = kNearThreads;
    out[2] = p.block_rows;
    out[3] = p.chunks;
    out[4] = p.chunk_rows;
    out[5] = p.lds;
    out[6] = p.scratch;
    out[7] = p.words;
  }
  return 0;
}
