// gf2_dev_words.h -- the word-level device helpers that more than one LPN module uses (bkw, lf2, join, sums, near, weight, gather, draw,
// cover), one copy of each; a helper of one module alone stays in that module.  Included by the .hip files
// only.  The helpers above the workgroup sums are plain values and pointers without a thread index: tests/test_dev_words_cpu.py runs
// their text on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;

// ---- the key of a row

// where the key lies in a row: word w0 from bit s on, `two`: the window runs on into word w0 + 1 (then s > 0)
struct Gf2KeyWindow {
  int w0, s, b;
  bool two;
  u32 mask;
};

__device__ __forceinline__ Gf2KeyWindow gf2_key_window(int c0, int b) {
  Gf2KeyWindow w;
  w.w0 = c0 >> 6;
  w.s = c0 & 63;
  w.b = b;
  w.two = w.s + b > 64;
  w.mask = (1u << b) - 1;
  return w;
}

// bits [c0, c0 + b) of a row: one word, or two funnelled together when the window crosses a word boundary (b <= 30: never three);
// the second word is read only then, and no word at all for b == 0
__device__ __forceinline__ u32 gf2_row_key(const u64 *row, Gf2KeyWindow w) {
  u32 v = 0;
  if (w.b > 0) {
    u64 x = row[w.w0] >> w.s;
    if (w.two) x |= row[w.w0 + 1] << (64 - w.s);
    v = (u32)x & w.mask;
  }
  return v;
}

// ---- words and pairs of words

__device__ __forceinline__ u64 gf2_lo_hi(u32 lo, u32 hi) { return (u64)lo | ((u64)hi << 32); }

// two words of a row from word k on; vec: the rows of this operand start on 16-byte boundaries, so the pair is one 16-byte access
__device__ __forceinline__ void gf2_load2(const u64 *row, long long k, int vec, u64 &x0, u64 &x1) {
  if (vec) {
    const uint4 x = *reinterpret_cast<const uint4 *>(row + k);
    x0 = gf2_lo_hi(x.x, x.y);
    x1 = gf2_lo_hi(x.z, x.w);
  } else {
    x0 = row[k];
    x1 = row[k + 1];
  }
}

// the bits of word k of a row that are columns of [wc0, wc1); a word outside the range has none
__device__ __forceinline__ u64 gf2_word_mask(long long k, int wc0, int wc1) {
  const long long lo = 64 * k, hi = lo + 64;
  if (wc0 >= wc1 || wc1 <= lo || wc0 >= hi) return 0;
  u64 m = ~0ull;
  if (wc0 > lo) m &= ~0ull << (wc0 - lo);
  if (wc1 < hi) m &= ~0ull >> (hi - wc1);
  return m;
}

// the ones of word k of a row, value x, that lie in the columns [wc0, wc1): the first and the last word of the range are masked, a
// word outside it counts nothing.  (The four lines of gf2_word_mask once more, not a call of it: through the call five join kernels
// are given other registers, and nobody has measured that code)
__device__ __forceinline__ int gf2_word_weight(u64 x, long long k, int wc0, int wc1) {
  const long long lo = 64 * k, hi = lo + 64;
  if (wc0 >= wc1 || wc1 <= lo || wc0 >= hi) return 0;
  u64 m = ~0ull;
  if (wc0 > lo) m &= ~0ull << (wc0 - lo);
  if (wc1 < hi) m &= ~0ull >> (hi - wc1);
  return __popcll(x & m);
}

// the position of output j of a run: the largest q < n with pre[q] <= j, where pre[q] = the outputs of the positions before q
// (pre[0] == 0 <= j < the run's total).  Positions without outputs (pre[q] == pre[q + 1]) are never the answer.
__device__ __forceinline__ int gf2_find_position(const long long *pre, int n, long long j) {
  int lo = 0, hi = n;  // pre[lo] <= j, and hi == n or pre[hi] > j
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// ---- sums over a workgroup of WAVES waves

// the sum of `mine` over the lanes before this one, and (in *total) over all.  wave_sum: WAVES values in LDS.  Every lane calls it; a
// barrier lies inside, and the caller puts one before wave_sum is used again.
template <typename T, int WAVES>
__device__ __forceinline__ T gf2_block_scan(T mine, T *wave_sum, T *total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  T incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  T before = incl - mine, all = 0;
#pragma unroll
  for (int wv = 0; wv < WAVES; ++wv) {
    if (wv < wave) before += wave_sum[wv];
    all += wave_sum[wv];
  }
  *total = all;
  return before;
}

// ---- host: what a launcher asks before it lets a kernel use 16-byte accesses

// 16-byte accesses only where every row starts on a 16-byte boundary and a row has a pair of words
static inline int gf2_rows_aligned16(const void *M, long long ld, long long nrows, long long nw) {
  return nw > 1 && !(reinterpret_cast<uintptr_t>(M) & 15) && (!(ld & 1) || nrows == 1);
}
