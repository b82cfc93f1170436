// cover_host.cpp -- gf2_cover_code_named, gf2_cover_leaders, gf2_cover_reduce_dev and gf2_cover_plan (include/m4ri_hip_cover.h; kernel:
// gf2_cover.hip).  Every argument is checked before a device is required and before the first HIP call, so a
// bad call fails the same way with and without a device; the aliasing check comes last.  The reduction only enqueues on the caller's
// stream: no host synchronisation, no hipMalloc, no scratch (codes and segments travel as the kernel's argument).
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/m4ri_hip_cover.h"
#include "../dev_args.h"
#include "cover_plan.h"
#include "gf2_cover.h"

namespace {

const uint32_t kGolayG = 0xC75;   // x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1

int top_bit(uint32_t x) { return 31 - __builtin_clz(x); }

}  // namespace

extern "C" int gf2_cover_code_named(int kind, int param, gf2_cover_code *code) {
  if (!code) return -1;
  gf2_cover_code c;
  memset(&c, 0, sizeof c);
  switch (kind) {
    case GF2_COVER_IDENTITY:
    case GF2_COVER_DROP:
      if (param < 1 || param > GF2_COVER_MAX_N) return -1;
      c.n = param;
      c.k = kind == GF2_COVER_IDENTITY ? param : 0;
      break;
    case GF2_COVER_REPETITION:
      if (param < 2 || param > GF2_COVER_MAX_R + 1) return -1;
      c.n = param;
      c.k = 1;
      for (int t = 0; t < param - 1; ++t) c.h[t] = 1u | (1u << (1 + t));
      break;
    case GF2_COVER_HAMMING: {
      if (param < 2 || param > 5) return -1;
      const int r = param;
      c.n = (1 << r) - 1;
      c.k = c.n - r;
      int j = 0;
      for (uint32_t v = 1; v < (1u << r); ++v) {
        if (!(v & (v - 1))) continue;   // a power of two: a check column
        for (int t = 0; t < r; ++t) c.h[t] |= ((v >> t) & 1u) << j;
        ++j;
      }
      for (int t = 0; t < r; ++t) c.h[t] |= 1u << (c.k + t);
      break;
    }
    case GF2_COVER_GOLAY23: {
      if (param != 0) return -1;
      c.n = 23;
      c.k = 12;
      uint32_t rem = 1u << 11;   // x^(11 + i) mod g, from i = 0 on
      for (int i = 0; i < 12; ++i) {
        if (rem >> 11) rem ^= kGolayG;
        for (int t = 0; t < 11; ++t) c.h[t] |= ((rem >> t) & 1u) << i;
        rem <<= 1;
      }
      for (int t = 0; t < 11; ++t) c.h[t] |= 1u << (12 + t);
      break;
    }
    default:
      return -1;
  }
  *code = c;
  return 0;
}

extern "C" int gf2_cover_leaders(gf2_cover_code const *code, uint32_t *leaders, int *radius) {
  if (!code || cover_code_fault(*code)) return -1;
  if (radius) *radius = 0;
  const int n = code->n, k = code->k, r = n - k;
  if (k == 0) return 0;
  if (!leaders) return -1;
  leaders[0] = 0;
  if (r == 0) return 0;
  uint32_t col[GF2_COVER_MAX_N];   // the syndrome of every unit pattern
  for (int j = 0; j < n; ++j) {
    col[j] = 0;
    for (int t = 0; t < r; ++t) col[j] |= ((code->h[t] >> j) & 1u) << t;
  }
  // By weight: a leader of weight w + 1 is a leader of weight w plus one bit above its top bit.  One pass over the syndromes per weight.
  const uint32_t size = 1u << r;
  std::vector<unsigned char> weight(size, 255);
  weight[0] = 0;
  uint32_t found = 1;
  int w = 0;
  for (; found < size; ++w) {
    for (uint32_t s = 0; s < size; ++s) {
      if (weight[s] != w) continue;
      const uint32_t e = leaders[s];
      for (int j = e ? top_bit(e) + 1 : 0; j < n; ++j) {
        const uint32_t s2 = s ^ col[j], e2 = e | (1u << j);
        if (weight[s2] == 255) {
          weight[s2] = (unsigned char)(w + 1);
          leaders[s2] = e2;
          ++found;
        } else if (weight[s2] == w + 1 && e2 < leaders[s2]) {
          leaders[s2] = e2;
        }
      }
    }
    if (w > n) return -1;   // cannot happen: the check columns alone reach every syndrome
  }
  if (radius) *radius = w;
  return 0;
}

extern "C" int gf2_cover_plan(int nrows, int p_ncols, gf2_cover_code const *codes, int ncodes, const unsigned char *seg_code, int nseg,
                              long long out[8]) {
  const CoverPlan p = cover_plan(nrows, p_ncols, codes, ncodes, seg_code, nseg);
  if (p.variant < 0) return -1;
  if (out) {
    out[0] = kCoverThreads;
    out[1] = p.lds;
    out[2] = kCoverThreads;
    out[3] = p.lanes;
    out[4] = p.K;
    out[5] = p.bits;
    out[6] = p.table_words;
    out[7] = p.blocks;
  }
  return p.variant;
}

extern "C" int gf2_cover_reduce_dev(gf2_dmat *D, gf2_dmat const *P, int c0, gf2_cover_code const *codes, int ncodes,
                                    const unsigned char *seg_code, int nseg, const uint32_t *const *leaders, int *dist, void *stream) {
  static const char fn[] = "gf2_cover_reduce_dev";
  if (gf2_check_mat(fn, "P", P)) return -1;
  if (gf2_check_mat(fn, "D", D)) return -1;
  GF2_RC(gf2_refuse_misaligned(fn, "dist", dist, 4));
  if (nseg < 0 || nseg > GF2_COVER_MAX_SEGS)
    return gf2_bad_arg(fn, "nseg = " + std::to_string(nseg) + " is outside 0 <= nseg <= " + std::to_string(GF2_COVER_MAX_SEGS));
  if (ncodes < (nseg ? 1 : 0) || ncodes > GF2_COVER_MAX_CODES)
    return gf2_bad_arg(fn, "ncodes = " + std::to_string(ncodes) + " is outside 1 <= ncodes <= " + std::to_string(GF2_COVER_MAX_CODES) +
                               " (0 only with nseg == 0)");
  if (ncodes > 0) GF2_RC(gf2_refuse_null(fn, "codes", codes));
  if (nseg > 0) GF2_RC(gf2_refuse_null(fn, "seg_code", seg_code));
  const uint32_t *table[GF2_COVER_MAX_CODES] = {nullptr};   // of the codes that have one and that a segment uses
  bool used[GF2_COVER_MAX_CODES] = {false};
  long long K = 0, bits = 0;
  for (int j = 0; j < nseg; ++j) {
    if (seg_code[j] >= ncodes)
      return gf2_bad_arg(fn, "seg_code[" + std::to_string(j) + "] = " + std::to_string((int)seg_code[j]) + " is not below ncodes = " +
                                 std::to_string(ncodes));
    used[seg_code[j]] = true;
  }
  long long table_words = 0;
  for (int c = 0; c < ncodes; ++c) {
    if (const int fault = cover_code_fault(codes[c])) return gf2_bad_arg(fn, "codes[" + std::to_string(c) + "]: " + cover_fault_text(fault));
    if (!cover_has_table(codes[c])) continue;
    if (used[c]) {
      const std::string name = "leaders[" + std::to_string(c) + "]";
      GF2_RC(gf2_refuse_null(fn, "leaders", leaders));
      GF2_RC(gf2_check_ptr(fn, name, leaders[c], 4));
      table[c] = leaders[c];
    }
    table_words += 1ll << (codes[c].n - codes[c].k);
  }
  if (table_words > GF2_COVER_MAX_LEADERS)
    return gf2_bad_arg(fn, "the tables hold " + std::to_string(table_words) + " words, above GF2_COVER_MAX_LEADERS = " +
                               std::to_string((int)GF2_COVER_MAX_LEADERS) + " (the sum of 2^r over the codes that have a table)");
  for (int j = 0; j < nseg; ++j) {
    K += codes[seg_code[j]].k;
    bits += codes[seg_code[j]].n;
  }
  if (c0 < 0 || c0 + bits > P->ncols)
    return gf2_bad_arg(fn, "the window [c0, c0 + sum of n) = [" + std::to_string(c0) + ", " + std::to_string(c0 + bits) + ") is outside P (" +
                               std::to_string(P->ncols) + " columns)");
  if (D->ncols != K)
    return gf2_bad_arg(fn, "D has " + std::to_string(D->ncols) + " columns, the segments have K = " + std::to_string(K) +
                               " message bits: D->ncols must equal K");
  if (D->nrows != P->nrows)
    return gf2_bad_arg(fn, "D has " + std::to_string(D->nrows) + " rows, P " + std::to_string(P->nrows) + ": D->nrows must equal P->nrows");
  // aliasing, last
  GF2_RC(gf2_refuse_overlap(fn, "D", D, "P", P));
  const long long dist_bytes = dist ? 4ll * P->nrows : 0;
  if (dist && gf2_range_meets_mat(dist, dist_bytes, P)) return gf2_bad_arg(fn, "dist and P overlap: the address range of dist may not meet P's");
  if (dist && gf2_range_meets_mat(dist, dist_bytes, D)) return gf2_bad_arg(fn, "dist and D overlap: the address range of dist may not meet D's");
  for (int c = 0; c < ncodes; ++c) {
    if (!table[c]) continue;
    const long long bytes = 4ll << (codes[c].n - codes[c].k);
    const std::string name = "leaders[" + std::to_string(c) + "]";
    if (gf2_range_meets_mat(table[c], bytes, D)) return gf2_bad_arg(fn, name + " and D overlap: a table may not meet the address range of D");
    if (gf2_ranges_meet(table[c], bytes, dist, dist_bytes))
      return gf2_bad_arg(fn, name + " and dist overlap: a table may not meet the address range of dist");
  }
  GF2_RC(gf2_require_device_for(fn));
  if (P->nrows == 0) return 0;
  if (K == 0 && !dist) return 0;   // nothing to write
  const hipError_t e = gf2k_cover_reduce(P->data, P->ld, P->nrows, P->ncols, c0, codes, ncodes, seg_code, nseg, table, D->data, D->ld, dist, -1, static_cast<hipStream_t>(stream));
  return gf2_hip_rc(e, fn);
}
