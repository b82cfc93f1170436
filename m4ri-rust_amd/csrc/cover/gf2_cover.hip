// gf2_cover.hip -- the covering-code reduction on the device (include/m4ri_hip_cover.h; host side and contract: cover_host.cpp; plan:
// cover_plan.h).
//
//   gf2_cover_kernel<staged>:  D[i] = the messages of the blocks of row i of P, dist[i] = the weight of what was removed
//
// A streaming map: every row depends on itself alone, every word of D and of dist has one writer, so the results are the same bits in
// every run.  The segment layout is the same for every row: which code, which block offset, which shift and mask are wave-uniform and
// come from the kernel argument (scalar loads, scalar arithmetic); only the row's bits are per lane.
//
// A workgroup copies the leader tables into LDS once and then loops over passes of kCoverThreads rows, a lane per row.  A block is read
// and decoded by cover_block alone: extract (one word, or two funnelled together), syndrome (r AND / popcount pairs against the check
// rows, which sit in scalar registers), one 4-byte LDS read of the leader, message and weight.  The messages are packed into 64-bit
// words in registers and stored as they fill up.
//
// staged: the window of a row touches few words (cover_plan.h).  The workgroup first copies those words of its rows into LDS, `lanes`
// lanes per row and a word per lane, so that a wave reads consecutive words of consecutive rows; the lanes then decode from LDS, rows
// an odd number of words apart (no bank conflict between the lanes of a wave).  Not staged: a lane reads the words of its row from
// global memory as its blocks need them.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <set>
#include <utility>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "cover_plan.h"
#include "gf2_cover.h"

namespace {

// What a launch carries as its kernel argument: the codes, the segments and where every table lies (in device memory and, in words,
// in the workgroup's LDS).  A code is sixteen words, so that one scalar load brings all of it: the check rows -- the rows from r on
// are ZERO, so that the syndrome needs no test per row -- and toff, the table's place in LDS (< 0: code c has no table, or no segment
// uses it).  A segment is 16 bits, two to a word (scalar loads know no bytes): its code, and that code's n and k once more, so that
// a segment's shape does not wait for the code.
struct CoverCodeArg {
  u32 h[GF2_COVER_MAX_R];
  int toff, n, k, pad;
};
struct CoverArgs {
  CoverCodeArg code[GF2_COVER_MAX_CODES];
  const u32 *table[GF2_COVER_MAX_CODES];
  u32 seg[GF2_COVER_MAX_SEGS / 2];
  int nseg, ncodes;
};
constexpr int kSegCodeBits = 4, kSegLenBits = 6;   // code | n << 4 | k << 10: sixteen bits
constexpr u32 kSegCodeMask = (1u << kSegCodeBits) - 1;

// segment j of the launch, segment 0 from nseg on
__device__ __forceinline__ u32 cover_seg(const CoverArgs &a, int j) {
  if (j >= a.nseg) j = 0;
  return a.seg[j >> 1] >> ((j & 1) * 16);
}

struct CoverBlock {
  u32 msg;  // (a ^ e) & mask(k)
  int wt;   // popcount(e)
};

// bit t of the syndrome of a, in its place: parity(a & h[t])
__host__ __device__ __forceinline__ u32 cover_syn_bit(u32 a, const u32 *h, int t) { return (u32)(__builtin_popcount(a & h[t]) & 1) << t; }

// The block a = bits [o, o + n) of `row` (1 <= n <= 32: at most two words, the second is read only when the block runs on into it),
// decoded by the [n, k] code with the check rows h[0 .. GF2_COVER_MAX_R), ZERO from row n - k on, and the table `leaders` (neither is
// read for k == 0 or k == n).  The syndrome takes the check rows four at a time: straight-line code on scalar operands.
__host__ __device__ __forceinline__ CoverBlock cover_block(const u64 *row, long long o, int n, int k, const u32 *h, const u32 *leaders) {
  const long long w0 = o >> 6;
  const int s = (int)(o & 63);
  u64 x = row[w0] >> s;
  if (s + n > 64) x |= row[w0 + 1] << (64 - s);
  const u32 mask_n = 0xFFFFFFFFu >> (32 - n);
  const u32 a = (u32)x & mask_n;
  const int r = n - k;
  u32 e;
  if (r == 0) {
    e = 0;
  } else if (k == 0) {
    e = a;
  } else {
    u32 syn = cover_syn_bit(a, h, 0) | cover_syn_bit(a, h, 1) | cover_syn_bit(a, h, 2) | cover_syn_bit(a, h, 3);
    if (r > 4) {
      syn |= cover_syn_bit(a, h, 4) | cover_syn_bit(a, h, 5) | cover_syn_bit(a, h, 6) | cover_syn_bit(a, h, 7);
      if (r > 8) syn |= cover_syn_bit(a, h, 8) | cover_syn_bit(a, h, 9) | cover_syn_bit(a, h, 10) | cover_syn_bit(a, h, 11);
    }
    e = leaders[syn] & mask_n;
  }
  CoverBlock b;
  b.msg = k ? (a ^ e) & (0xFFFFFFFFu >> (32 - k)) : 0;
  b.wt = __builtin_popcount(e);
  return b;
}

// the next word of a row of D: alone, or -- vec -- held back until its pair is complete
__device__ __forceinline__ void cover_emit(u64 *drow, long long &qw, u64 x, u64 &held, int vec) {
  if (!vec)
    drow[qw] = x;
  else if (qw & 1)
    *reinterpret_cast<uint4 *>(drow + qw - 1) = make_uint4((u32)held, (u32)(held >> 32), (u32)x, (u32)(x >> 32));
  else
    held = x;
  ++qw;
}

// stride: words between the staged rows of a workgroup (odd, at least the words of the window); lanes = 1 << lanes_log2 per row copy
// them.  nwd: words of a row of D.  vec_d: every row of D starts on a 16-byte boundary and has a pair of words.
template <bool STAGED>
__global__ void __launch_bounds__(kCoverThreads) gf2_cover_kernel(const u64 *P, long long ld, long long nrows, int c0, long long bits,
                                                                  CoverArgs a, int stride, int lanes_log2, u64 *D, long long ldd, int nwd,
                                                                  int *dist, int vec_d) {
  extern __shared__ u64 cover_lds[];
  u64 *stage = cover_lds;
  u32 *tab = reinterpret_cast<u32 *>(cover_lds + (STAGED ? kCoverThreads * stride : 0));
  const int tid = threadIdx.x;
  for (int c = 0; c < a.ncodes; ++c) {
    if (a.code[c].toff < 0) continue;
    const int size = 1 << (a.code[c].n - a.code[c].k);
    const u32 *src = a.table[c];
    for (int i = tid; i < size; i += kCoverThreads) tab[a.code[c].toff + i] = src[i];
  }
  if (!STAGED) __syncthreads();   // the staged passes have a barrier of their own before the first look-up
  // the words of a row that hold a bit of the window: [wfirst, wfirst + wcount)
  const long long wfirst = c0 >> 6;
  const int wcount = bits > 0 ? (int)(((c0 + bits - 1) >> 6) - wfirst + 1) : 0;
  const long long o0 = STAGED ? (c0 & 63) : c0;   // the staged words start with word wfirst
  for (long long row0 = (long long)blockIdx.x * kCoverThreads; row0 < nrows; row0 += (long long)gridDim.x * kCoverThreads) {
    const long long r = row0 + tid;
    const u64 *row = P + r * ld;
    if (STAGED) {
      const int sub = tid & ((1 << lanes_log2) - 1);
      if (sub < wcount)
        for (int q = tid >> lanes_log2; q < kCoverThreads && row0 + q < nrows; q += kCoverThreads >> lanes_log2)
          stage[q * stride + sub] = P[(row0 + q) * ld + wfirst + sub];
      __syncthreads();
      row = stage + tid * stride;
    }
    if (r < nrows) {
      u64 *drow = D + r * ldd;
      long long o = o0, qw = 0;
      int qbit = 0, wt = 0;
      u64 acc = 0, held = 0;
      // the scalar loads run ahead of the blocks: the segment after next and the code of the next one are asked for while this one
      // is decoded (segments past the last read as segment 0, which is harmless)
      u32 sd = cover_seg(a, 0), sd1 = cover_seg(a, 1);
      CoverCodeArg cd = a.code[sd & kSegCodeMask];
      for (int j = 0; j < a.nseg; ++j) {
        const u32 sd2 = cover_seg(a, j + 2);
        const CoverCodeArg cd1 = a.code[sd1 & kSegCodeMask];
        const int n = (sd >> kSegCodeBits) & ((1 << kSegLenBits) - 1), k = (sd >> (kSegCodeBits + kSegLenBits)) & ((1 << kSegLenBits) - 1);
        const CoverBlock b = cover_block(row, o, n, k, cd.h, tab + cd.toff);
        sd = sd1, sd1 = sd2, cd = cd1;
        o += n;
        wt += b.wt;
        if (k) {
          acc |= (u64)b.msg << qbit;
          if (qbit + k >= 64) {
            cover_emit(drow, qw, acc, held, vec_d);
            acc = qbit + k > 64 ? (u64)b.msg >> (64 - qbit) : 0;
          }
          qbit = (qbit + k) & 63;
        }
      }
      if (qbit) cover_emit(drow, qw, acc, held, vec_d);   // the last word: its excess bits are zero
      if (vec_d && (nwd & 1)) drow[nwd - 1] = held;       // a last word without a pair
      if (dist) dist[r] = wt;
    }
    if (STAGED) __syncthreads();   // before the next pass overwrites the staged words
  }
}

// the dynamic-LDS limit of a kernel is per device and costs host time: once per (kernel, device)
hipError_t cover_lds_limit_once(const void *kernel, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void *, int>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({kernel, dev})) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.insert({kernel, dev});
  return e;
}

constexpr int kCoverMostLds = 4 * GF2_COVER_MAX_LEADERS + 8 * kCoverThreads * (kCoverStageWords | 1);

}  // namespace

extern "C" hipError_t gf2k_cover_reduce(const u64 *P, long long ld, int nrows, int p_ncols, int c0, const gf2_cover_code *codes, int ncodes,
                                        const unsigned char *seg_code, int nseg, const u32 *const *tables, u64 *D, long long ldd, int *dist,
                                        int variant, hipStream_t stream) {
  const CoverPlan plan = cover_plan(nrows, p_ncols, codes, ncodes, seg_code, nseg);
  if (plan.variant < 0 || nrows <= 0 || c0 < 0 || c0 + plan.bits > p_ncols) return hipErrorInvalidValue;
  if (variant < 0) variant = plan.variant;
  if (variant == 1 && (plan.span < 1 || plan.span > kCoverStageWords)) return hipErrorInvalidValue;
  if (variant != 0 && variant != 1) return hipErrorInvalidValue;
  CoverArgs a;
  memset(&a, 0, sizeof a);
  a.nseg = nseg;
  a.ncodes = ncodes;
  bool used[GF2_COVER_MAX_CODES] = {false};
  for (int j = 0; j < nseg; ++j) {
    const int c = seg_code[j];
    used[c] = true;
    a.seg[j >> 1] |= (u32)(c | codes[c].n << kSegCodeBits | codes[c].k << (kSegCodeBits + kSegLenBits)) << ((j & 1) * 16);
  }
  int words = 0;
  for (int c = 0; c < ncodes; ++c) {
    a.code[c].n = codes[c].n;
    a.code[c].k = codes[c].k;
    a.code[c].toff = -1;
    if (!cover_has_table(codes[c])) continue;
    for (int t = 0; t < codes[c].n - codes[c].k; ++t) a.code[c].h[t] = codes[c].h[t];   // the rows behind stay zero
    if (used[c]) {
      if (!tables || !tables[c]) return hipErrorInvalidValue;
      a.table[c] = tables[c];
      a.code[c].toff = words;
    }
    words += 1 << (codes[c].n - codes[c].k);
  }
  const int nwd = (int)((plan.K + 63) >> 6);
  const int vec_d = gf2_rows_aligned16(D, ldd, nrows, nwd);
  const int stride = plan.span | 1;
  int lanes_log2 = 0;
  while ((1 << lanes_log2) < plan.span) ++lanes_log2;
  const int lds = (int)(4 * plan.table_words) + (variant == 1 ? 8 * kCoverThreads * stride : 0);
  const dim3 grid((unsigned)plan.blocks), block(kCoverThreads);
  const void *kernel = variant == 1 ? reinterpret_cast<const void *>(&gf2_cover_kernel<true>) : reinterpret_cast<const void *>(&gf2_cover_kernel<false>);
  const hipError_t e = cover_lds_limit_once(kernel, kCoverMostLds);
  if (e != hipSuccess) return e;
  if (variant == 1)
    hipLaunchKernelGGL((gf2_cover_kernel<true>), grid, block, lds, stream, P, ld, (long long)nrows, c0, plan.bits, a, stride, lanes_log2, D, ldd,
                       nwd, dist, vec_d);
  else
    hipLaunchKernelGGL((gf2_cover_kernel<false>), grid, block, lds, stream, P, ld, (long long)nrows, c0, plan.bits, a, stride, lanes_log2, D, ldd,
                       nwd, dist, vec_d);
  return hipGetLastError();
}
