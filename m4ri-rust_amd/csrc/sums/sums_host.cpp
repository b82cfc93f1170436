// sums_host.cpp -- gf2_subset_sums_dev, gf2_unrank_subsets_dev, the host routines of the order and gf2_subset_sums_plan
// (include/m4ri_hip_sums.h; kernels: gf2_sums.hip; order and plan: sums_plan.h).  Every argument is checked
// before a device is required and before the first HIP call, so a bad call fails the same way with and without a device; the aliasing
// check comes last, and a call that has nothing to write returns without a device.  The device entries only enqueue on the caller's
// stream: no host synchronisation, no hipMalloc, no scratch.
#include <stdint.h>

#include <string>

#include "../../../include/m4ri_hip_sums.h"
#include "../dev_args.h"
#include "gf2_sums.h"
#include "sums_plan.h"

namespace {

int check_p(const char *fn, int p) {
  if (p >= 1 && p <= kSumsMaxP) return 0;
  return gf2_bad_arg(fn, "p = " + std::to_string(p) + " is outside 1 <= p <= " + std::to_string(kSumsMaxP));
}

// C(n, p) -> *total, or the refusal of a count that passes 2^62
int check_count(const char *fn, long long n, int p, long long *total) {
  *total = sums_count(n, p);
  if (*total >= 0) return 0;
  return gf2_bad_arg(fn, "C(" + std::to_string(n) + ", " + std::to_string(p) + ") passes 2^62: the count of the subsets overflows");
}

}  // namespace

extern "C" int gf2_subset_sums_dev(gf2_dmat *D, gf2_dmat const *S, gf2_dmat const *base, int p, long long rank0, int *idx, int *wt, int wc0,
                                   int wc1, void *stream) {
  static const char fn[] = "gf2_subset_sums_dev";
  if (gf2_check_mat(fn, "S", S)) return -1;
  if (base && gf2_check_mat(fn, "base", base)) return -1;
  if (gf2_check_mat(fn, "D", D, /*unstored_ok=*/true)) return -1;
  if (base && base->nrows != 1) return gf2_bad_arg(fn, "base has " + std::to_string(base->nrows) + " rows: base is null or one row");
  if (D->ncols != S->ncols || (base && base->ncols != S->ncols))
    return gf2_bad_arg(fn, "S has " + std::to_string(S->ncols) + " columns, D " + std::to_string(D->ncols) +
                               (base ? ", base " + std::to_string(base->ncols) : std::string()) +
                               ": S->ncols, D->ncols and base->ncols must be equal");
  GF2_RC(check_p(fn, p));
  long long total;
  GF2_RC(check_count(fn, S->nrows, p, &total));
  if (rank0 < 0 || rank0 > total || D->nrows > total - rank0)
    return gf2_bad_arg(fn, "the ranks [rank0, rank0 + D->nrows) = [" + std::to_string(rank0) + ", " + std::to_string(rank0) + " + " +
                               std::to_string(D->nrows) + ") are outside [0, C(n, p)) = [0, " + std::to_string(total) + ")");
  GF2_RC(gf2_refuse_misaligned(fn, "idx", idx, 4));
  GF2_RC(gf2_refuse_misaligned(fn, "wt", wt, 4));
  GF2_RC(gf2_check_weight_range(fn, S->ncols, wc0, wc1));
  const bool stored = D->data != nullptr && D->ncols > 0;
  if (D->nrows > 0 && !D->data && !idx && !wt)
    return gf2_bad_arg(fn, "D.data is null and so are idx and wt: rows that are not stored need idx or wt");
  // aliasing, last.  S and base are only read: they may overlap
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "S", S));
  if (base) GF2_RC(gf2_refuse_overlap(fn, "D", D, "base", base));
  const Gf2FlatArray arrays[2] = {{"idx", idx, 4ll * p * D->nrows}, {"wt", wt, 4ll * D->nrows}};
  const Gf2NamedMat mats[3] = {{"S", S}, {"base", base}, {"D", D}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 2, mats, 3));
  if (D->nrows == 0 || (!stored && !idx && !wt)) return 0;  // nothing to write (the second: rows without a word, and no array)
  GF2_RC(gf2_require_device_for(fn));
  const hipError_t e = gf2k_subset_sums(S->data, S->ld, S->nrows, base ? base->data : nullptr, S->ncols, p, rank0, D->nrows,
                                        stored ? D->data : nullptr, D->ld, idx, wt, wc0, wc1, 0, static_cast<hipStream_t>(stream));
  return gf2_hip_rc(e, fn);
}

extern "C" int gf2_unrank_subsets_dev(const int *ranks, int count, long long rank0, int p, int n, int *idx, int *bad, void *stream) {
  static const char fn[] = "gf2_unrank_subsets_dev";
  if (count < 0 || n < 0) return gf2_bad_arg(fn, count < 0 ? "count is negative" : "n is negative");
  GF2_RC(check_p(fn, p));
  long long total;
  GF2_RC(check_count(fn, n, p, &total));
  if (rank0 < 0 || rank0 > (long long)kSumsMaxCount)
    return gf2_bad_arg(fn, "rank0 = " + std::to_string(rank0) + " is outside 0 <= rank0 <= 2^62");
  if (count > 0) {
    GF2_RC(gf2_check_ptr(fn, "ranks", ranks, 4));
    GF2_RC(gf2_check_ptr(fn, "idx", idx, 4));
  }
  GF2_RC(gf2_refuse_misaligned(fn, "bad", bad, 4));
  const Gf2FlatArray arrays[3] = {{"ranks", ranks, 4ll * count}, {"idx", idx, 4ll * p * count}, {"bad", count > 0 ? bad : nullptr, 4}};
  GF2_RC(gf2_refuse_array_overlaps(fn, arrays, 3, nullptr, 0));
  if (count == 0) return 0;
  GF2_RC(gf2_require_device_for(fn));
  return gf2_hip_rc(gf2k_unrank_subsets(ranks, count, rank0, p, n, idx, bad, static_cast<hipStream_t>(stream)), fn);
}

extern "C" long long gf2_subset_count(int n, int p) { return sums_count(n, p); }

extern "C" long long gf2_subset_rank(const int *c, int p) {
  if (p < 1 || p > kSumsMaxP || !c) return -1;
  unsigned u[4] = {kSumsNone, kSumsNone, kSumsNone, kSumsNone};
  for (int i = 0; i < p; ++i) {
    if (c[i] < 0 || (i && c[i] <= c[i - 1])) return -1;
    u[i] = (unsigned)c[i];
  }
  if (sums_count((long long)c[p - 1] + 1, p) < 0) return -1;  // the rank would pass 2^62
  return (long long)sums_rank(u, p);
}

extern "C" int gf2_subset_unrank(long long rank, int p, int *c) {
  if (p < 1 || p > kSumsMaxP || !c || rank < 0 || rank >= (long long)kSumsMaxCount) return -1;
  unsigned u[4];
  if (sums_unrank((unsigned long long)rank, p, kSumsNone, u) != 0 || u[p - 1] > 0x7FFFFFFFu) return -1;
  for (int i = 0; i < p; ++i) c[i] = (int)u[i];
  return 0;
}

extern "C" int gf2_subset_sums_plan(int n, int ncols, int p, long long count, long long out[6]) {
  const SumsPlan s = sums_plan(n, ncols, p, count);
  if (s.id < 0 || count > 0x7FFFFFFFll) return -1;
  if (out) {
    out[0] = kSumsThreads;
    out[1] = s.ranks;
    out[2] = s.lanes;
    out[3] = s.lds;
    out[4] = s.groups;
    out[5] = 0;  // no scratch
  }
  return s.id;
}
