// gather_host.cpp -- gf2_gather_rows_dev, gf2_gather_cols_dev and gf2_gather_cols_plan (include/m4ri_hip_gather.h; kernels:
// gf2_gather.hip).  Every argument is checked before a device is required and before the first HIP call, so a
// bad call fails the same way with and without a device, and an empty D returns without one.  Both entries only enqueue on the caller's
// stream: no host synchronisation, no hipMalloc (the composed column route draws on the stream's scratch arena).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_gather.h"
#include "../dev_args.h"
#include "../gf2_kernels.h"
#include "gather_plan.h"
#include "gf2_gather.h"

namespace {

// 0: go ahead; 1: nothing to do; -1: refused (gf2_last_error is set).  count: the ints idx holds
int check_call(const char *fn, gf2_dmat *D, gf2_dmat const *S, const int *idx, long long count, const int *bad, bool rows) {
  if (gf2_check_mat(fn, "D", D) || gf2_check_mat(fn, "S", S)) return -1;
  if (rows ? D->ncols != S->ncols : D->nrows != S->nrows)
    return gf2_bad_arg(fn, rows ? "shape mismatch: D and S must have equal column counts (D.ncols != S.ncols)"
                                : "shape mismatch: D and S must have equal row counts (D.nrows != S.nrows)");
  if (D->nrows == 0 || D->ncols == 0) return 1;
  GF2_RC(gf2_check_ptr(fn, "idx", idx, 4));
  if (bad) GF2_RC(gf2_refuse_misaligned(fn, "bad", bad, 4));
  if (gf2_refuse_overlap(fn, "D", D, "S", S)) return -1;
  if (gf2_range_meets_mat(idx, 4 * count, D)) return gf2_bad_arg(fn, "idx and D overlap: the address range of idx may not meet D's");
  if (bad && gf2_range_meets_mat(bad, 4, D)) return gf2_bad_arg(fn, "bad and D overlap: the address of bad may not lie in D's address range");
  return 0;
}

}  // namespace

extern "C" int gf2_gather_rows_dev(gf2_dmat *D, gf2_dmat const *S, const int *idx, int accumulate, int *bad, void *stream) {
  static const char fn[] = "gf2_gather_rows_dev";
  if (int rc = check_call(fn, D, S, idx, D ? D->nrows : 0, bad, true)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device());
  const hipError_t e = gf2k_gather_rows(D->data, D->ld, S->data, S->ld, D->nrows, S->nrows, D->ncols, idx, accumulate, bad,
                                        static_cast<hipStream_t>(stream));
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_gather_cols_dev(gf2_dmat *D, gf2_dmat const *S, const int *idx, int *bad, void *stream) {
  static const char fn[] = "gf2_gather_cols_dev";
  if (int rc = check_call(fn, D, S, idx, D ? D->ncols : 0, bad, false)) return rc < 0 ? rc : 0;
  GF2_RC(gf2_require_device());
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GatherColsPlan plan = gather_cols_plan(D->nrows, S->ncols, D->ncols);
  if (plan.path == 0) {
    const hipError_t e = gf2k_gather_cols(D->data, D->ld, D->ncols, S->data, S->ld, S->ncols, D->nrows, idx, bad, s);
    return gf2_hip_rc(e, fn);
  }
  // composed: T = S^T, G[j] = T[idx[j]], D = G^T, all on s; the two scratch matrices stay with the stream for the next call
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  const long long ldt = gather_ld_for(D->nrows);
  void *pt = nullptr, *pg = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)(8 * ldt * S->ncols), &pt, GF2_SLOT_GATHER_TRANSPOSED));
  GF2_RC(gf2_stream_scratch(s, (size_t)(8 * ldt * D->ncols), &pg, GF2_SLOT_GATHER_ROWS));
  uint64_t *T = static_cast<uint64_t *>(pt), *G = static_cast<uint64_t *>(pg);
  hipError_t e = gf2k_transpose(T, ldt, S->data, S->ld, S->nrows, S->ncols, s);
  if (e == hipSuccess) e = gf2k_gather_rows(G, ldt, T, ldt, D->ncols, S->ncols, D->nrows, idx, 0, bad, s);
  if (e == hipSuccess) e = gf2k_transpose(D->data, D->ld, G, ldt, D->ncols, D->nrows, s);
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_gather_cols_plan(int nrows, int s_ncols, int d_ncols, long long out[4]) {
  const GatherColsPlan plan = gather_cols_plan(nrows, s_ncols, d_ncols);
  if (out) {
    out[0] = plan.threads;
    out[1] = plan.lds_bytes;
    out[2] = plan.rows;
    out[3] = plan.scratch;
  }
  return plan.path;
}
