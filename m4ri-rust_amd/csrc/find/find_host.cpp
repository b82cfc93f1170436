// find_host.cpp -- gf2_find_rows_dev and gf2_find_rows_plan (include/m4ri_hip_find.h; kernels: gf2_find.hip).
// Every argument is checked before a device is required and before the first HIP call, so a bad call fails the same way with and
// without a device; the aliasing check comes last.  The entry only enqueues on the caller's stream: no host synchronisation, no
// hipMalloc (the table comes from the stream's scratch arena and is filled by the first launch of the call).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_find.h"
#include "../dev_args.h"
#include "find_plan.h"
#include "gf2_find.h"

extern "C" int gf2_find_rows_dev(gf2_dmat const *A, gf2_dmat const *B, int c0, int c1, int *idx, int *mult, int *count, void *stream) {
  static const char fn[] = "gf2_find_rows_dev";
  if (gf2_check_mat(fn, "A", A)) return -1;
  GF2_RC(gf2_check_mat(fn, "B", B));
  const int ncols = A->ncols < B->ncols ? A->ncols : B->ncols;
  if (c0 < 0 || c0 > c1 || c1 > ncols)
    return gf2_bad_arg(fn, "the columns [c0, c1) = [" + std::to_string(c0) + ", " + std::to_string(c1) + ") are outside 0 <= c0 <= c1 <= " +
                               std::to_string(ncols) + " columns (A has " + std::to_string(A->ncols) + ", B " + std::to_string(B->ncols) + ")");
  GF2_RC(gf2_check_ptr(fn, "idx", idx, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "mult", mult, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "count", count, 4));
  // aliasing, last
  const Gf2FlatArray arrays[3] = {{"idx", idx, 4ll * A->nrows}, {"mult", mult, 4ll * A->nrows}, {"count", count, 4}};
  const Gf2NamedMat mats[2] = {{"A", A}, {"B", B}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 3, mats, 2));
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->nrows == 0 || B->nrows == 0) {  // no table: idx all -1, mult all 0, *count = 0; without rows of A only the count
    if (A->nrows > 0) {
      GF2_RC(gf2_hip_rc(hipMemsetAsync(idx, 0xFF, 4ull * A->nrows, s), fn));
      if (mult) GF2_RC(gf2_hip_rc(hipMemsetAsync(mult, 0, 4ull * A->nrows, s), fn));
    }
    return count ? gf2_hip_rc(hipMemsetAsync(count, 0, 4, s), fn) : 0;
  }
  const FindPlan plan = find_plan(A->nrows, B->nrows, ncols, c0, c1);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *table = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.scratch, &table, GF2_SLOT_FIND));
  return gf2_hip_rc(gf2k_find_rows(A->data, A->ld, A->nrows, B->data, B->ld, B->nrows, c0, c1, table, idx, mult, count, s), fn);
}

extern "C" int gf2_find_rows_plan(int nrows_a, int nrows_b, int ncols, int c0, int c1, long long out[8]) {
  const FindPlan p = find_plan(nrows_a, nrows_b, ncols, c0, c1);
  if (p.slots < 0) return -1;
  if (out) {
    out[0] = p.slots;
    out[1] = kFindSlotBytes;
    out[2] = p.scratch;
    out[3] = p.launches;
    out[4] = p.build_rows;
    out[5] = p.lookup_rows;
    out[6] = p.wave;
    out[7] = p.words;
  }
  return p.slots > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)p.slots;
}
