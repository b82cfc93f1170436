// draw_host.cpp -- gf2_bernoulli_dev, gf2_bernoulli_block_dev, gf2_draw_indices_dev, gf2_draw_subsets_dev, gf2_draw_permutation_dev
// and gf2_draw_plan (include/m4ri_hip_draw.h; kernels: gf2_draw.hip).  Every argument is checked before a
// device is required and before the first HIP call, so a bad call fails the same way with and without a device; the aliasing check
// comes last.  The entries only enqueue on the caller's stream: no host synchronisation, no hipMalloc (the pair buffers and digit
// counts of the permutation's sort come from the stream's scratch arena and are written before they are read).
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_draw.h"
#include "../dev_args.h"
#include "../lf2/gf2_lf2.h"
#include "draw_plan.h"
#include "gf2_draw.h"
#include "philox.h"

namespace {

int check_n(const char *fn, int n) {
  return n >= 1 ? 0 : gf2_bad_arg(fn, "n = " + std::to_string(n) + " is outside 1 <= n <= 2^31 - 1");
}

int bernoulli(const char *fn, gf2_dmat *D, uint32_t thr, uint64_t seed, int64_t row0, int64_t col_word0, int full_ncols, int accumulate,
              void *stream) {
  if (gf2_check_mat(fn, "D", D)) return -1;
  if (row0 < 0 || col_word0 < 0 || full_ncols < 0)
    return gf2_bad_arg(fn, "row0 = " + std::to_string(row0) + ", col_word0 = " + std::to_string(col_word0) + ", full_ncols = " +
                               std::to_string(full_ncols) + ": none of them may be negative");
  const long long w = ((long long)D->ncols + 63) >> 6;
  const long long fullw = full_ncols > 0 ? ((long long)full_ncols + 63) >> 6 : w;
  if (full_ncols > 0 && col_word0 + w > fullw)
    return gf2_bad_arg(fn, "the words [col_word0, col_word0 + " + std::to_string(w) + ") of a row are outside the whole matrix (" +
                               std::to_string(fullw) + " words per row)");
  GF2_RC(gf2_require_device_for(fn));
  if (D->nrows == 0 || D->ncols == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (thr == 0)  // no bit is ever set: zero rows, or nothing to add
    return accumulate ? 0 : gf2_hip_rc(hipMemset2DAsync(D->data, 8 * (size_t)D->ld, 0, 8 * (size_t)w, (size_t)D->nrows, s), fn);
  return gf2_hip_rc(gf2k_bernoulli(D->data, D->ld, D->nrows, D->ncols, thr, seed, row0, fullw, col_word0, accumulate ? 1 : 0, s), fn);
}

}  // namespace

extern "C" int gf2_bernoulli_dev(gf2_dmat *D, uint32_t thr, uint64_t seed, int accumulate, void *stream) {
  return bernoulli("gf2_bernoulli_dev", D, thr, seed, 0, 0, 0, accumulate, stream);
}

extern "C" int gf2_bernoulli_block_dev(gf2_dmat *D, uint32_t thr, uint64_t seed, int64_t row0, int64_t col_word0, int full_ncols,
                                       int accumulate, void *stream) {
  return bernoulli("gf2_bernoulli_block_dev", D, thr, seed, row0, col_word0, full_ncols, accumulate, stream);
}

extern "C" int gf2_draw_indices_dev(int *idx, long long count, int n, uint64_t seed, void *stream) {
  static const char fn[] = "gf2_draw_indices_dev";
  GF2_RC(gf2_check_ptr(fn, "idx", idx, 4));
  if (count < 0) return gf2_bad_arg(fn, "count = " + std::to_string(count) + " is negative");
  GF2_RC(check_n(fn, n));
  GF2_RC(gf2_require_device_for(fn));
  if (count == 0) return 0;
  return gf2_hip_rc(gf2k_draw_indices(idx, count, (uint32_t)n, seed, static_cast<hipStream_t>(stream)), fn);
}

extern "C" int gf2_draw_subsets_dev(int *sub, int batch, int k, int n, uint64_t seed, int max_rounds, int *unfinished, void *stream) {
  static const char fn[] = "gf2_draw_subsets_dev";
  GF2_RC(gf2_check_ptr(fn, "sub", sub, 4));
  if (batch < 0) return gf2_bad_arg(fn, "batch = " + std::to_string(batch) + " is negative");
  if (k < 1 || k > kDrawSubsetMaxK)
    return gf2_bad_arg(fn, "k = " + std::to_string(k) + " is outside 1 <= k <= " + std::to_string(kDrawSubsetMaxK));
  GF2_RC(check_n(fn, n));
  if (2ll * k > n)
    return gf2_bad_arg(fn, "k = " + std::to_string(k) + ", n = " + std::to_string(n) + ": 2 k may not exceed n (a draw must settle with probability 1/2 at least)");
  if (max_rounds < 0 || max_rounds > kDrawSubsetMaxRounds)
    return gf2_bad_arg(fn, "max_rounds = " + std::to_string(max_rounds) + " is outside 0 <= max_rounds <= " + std::to_string(kDrawSubsetMaxRounds));
  GF2_RC(gf2_refuse_misaligned(fn, "unfinished", unfinished, 4));
  // aliasing, last
  if (unfinished && gf2_ranges_meet(sub, 4ll * batch * k, unfinished, 4))
    return gf2_bad_arg(fn, "sub and unfinished overlap: their address ranges may not meet");
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (unfinished) GF2_RC(gf2_hip_rc(hipMemsetAsync(unfinished, 0, 4, s), fn));  // the workgroups count behind this, on the same stream
  if (batch == 0) return 0;
  return gf2_hip_rc(gf2k_draw_subsets(sub, batch, k, (uint32_t)n, seed, max_rounds ? max_rounds : kDrawSubsetMaxRounds, unfinished, s), fn);
}

extern "C" int gf2_draw_permutation_dev(int *perm, int n, uint64_t seed, void *stream) {
  static const char fn[] = "gf2_draw_permutation_dev";
  GF2_RC(gf2_check_ptr(fn, "perm", perm, 4));
  if (n < 0) return gf2_bad_arg(fn, "n = " + std::to_string(n) + " is negative");
  GF2_RC(gf2_require_device_for(fn));
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Lf2Plan plan = draw_perm_plan(n);
  std::lock_guard<std::mutex> lk(gf2_enqueue_mu);  // another thread on the same stream would be handed the same scratch
  void *scratch = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)plan.sort_scratch, &scratch, GF2_SLOT_DRAW_PERM));
  const Lf2SortWork w = lf2_sort_work(scratch, plan);
  GF2_RC(gf2_hip_rc(gf2k_draw_perm_pairs(w.pairs[0], n, seed, s), fn));
  // the class sort on pairs from pass 0 on, not gf2_enqueue_class_sort: no matrix, the pairs go from one buffer to the other and the
  // last pass writes perm
  for (int pass = 0; pass < plan.passes; ++pass) {
    const bool last = pass == plan.passes - 1;
    const hipError_t e = gf2k_lf2_sort_pass(nullptr, 0, 0, kDrawPermKeyBits, w.pairs[pass & 1], n, pass, w.counts, w.parts,
                                            last ? nullptr : w.pairs[(pass + 1) & 1], last ? perm : nullptr, nullptr, s);
    GF2_RC(gf2_hip_rc(e, fn));
  }
  return 0;
}

extern "C" int gf2_draw_plan(int what, long long count_or_k, int n, uint32_t thr, long long out[4]) {
  long long o[4] = {0, 0, 0, 0};
  switch (what) {
    case GF2_DRAW_BERNOULLI:
      o[0] = draw_bernoulli_calls(thr);
      o[1] = kDrawThreads;
      o[2] = (long long)kDrawMaxBlocks * kDrawThreads;
      break;
    case GF2_DRAW_INDICES:
      if (count_or_k < 0 || n < 1) return -1;
      o[0] = (count_or_k + 1) >> 1;
      o[1] = kDrawThreads;
      o[2] = 2ll * kDrawMaxBlocks * kDrawThreads;
      break;
    case GF2_DRAW_SUBSETS: {
      const DrawSubsetPlan p = draw_subset_plan(count_or_k);
      if (p.per_group == 0 || n < 1 || 2 * count_or_k > n) return -1;
      o[0] = kDrawThreads;
      o[1] = p.lds_bytes;
      o[2] = p.per_group;
      o[3] = kDrawSubsetMaxRounds;
      break;
    }
    case GF2_DRAW_PERMUTATION: {
      if (n < 0) return -1;
      const Lf2Plan p = draw_perm_plan(n);
      o[0] = n ? p.sort_scratch : 0;
      o[1] = p.passes;
      o[2] = kDrawPermKeyBits;
      break;
    }
    default:
      return -1;
  }
  if (out)
    for (int i = 0; i < 4; ++i) out[i] = o[i];
  return 0;
}
