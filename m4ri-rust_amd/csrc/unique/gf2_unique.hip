// gf2_unique.hip -- the kernels between the passes of the class sort and the ascending compaction that make a row sort on any column
// range and the removal of duplicate rows (include/m4ri_hip_unique.h; host side and contract: unique_host.cpp; plan: unique_plan.h;
// DESIGN.md section 7.20).
//
//   sort, per window of up to 24 columns, least significant first:
//     pairs[i] = (the window's bits of row r, r), r in the current order    gf2_unique_rekey_kernel
//     the passes of the class sort on those pairs                           gf2k_lf2_sort_pass (lf2/gf2_lf2.hip), the last into order
//   heads, on the sorted order:
//     head[s] = s where rows order[s - 1] and order[s] differ on the        gf2_unique_heads_kernel
//     range (and for s == 0), else -1; the last head of every run
//     carry[run] = the last head of the runs before it                      gf2_unique_carry_kernel
//     head[s] = the last head at or below s                                 gf2_unique_fill_kernel
//   unique:
//     rep[order[s]] = order[head[s]], flags[i] = (rep[i] == i)              gf2_unique_rep_kernel
//     keep = the i with flags[i] == 1, ascending; *count                    gf2k_weight_select (weight/gf2_weight.hip)
//
// The bits of a window are read by gf2_row_key, the bits of a word of the range by gf2_word_mask (gf2_dev_words.h) alone.  Rows are
// read with 8-byte loads and 64-bit offsets: only the words that hold a column of the range, the first and the last of them masked.
//
// A head is a sorted position whose row differs from the one before it; the heads ascend, so "the last head at or below s" is a
// running maximum, taken inside a wave by shuffles, across the waves of a run through LDS and across the runs by the carries.  Position
// 0 is a head, so every maximum is one: a single class that spans every run is carried from run 0 to the last.
//
// Everything is integer arithmetic with one writer per output word and no atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_unique.h"
#include "unique_plan.h"

namespace {

// do two rows differ in a column of [c0, c1)?  [w0, w1): the words of a row that hold a column of the range (unique_plan.h); no
// other word is read, and none behind the first that differs
__device__ __forceinline__ bool unique_rows_differ(const u64 *a, const u64 *b, long long w0, long long w1, int c0, int c1) {
  for (long long k = w0; k < w1; ++k)
    if ((a[k] ^ b[k]) & gf2_word_mask(k, c0, c1)) return true;
  return false;
}

// the maximum of `mine` over the lanes before this one (-1 for lane 0 of the workgroup), and (in *total) over all.  wave_max:
// kUniqueWaves values in LDS.  Every lane calls it; a barrier lies inside, and the caller puts one before wave_max is used again.
__device__ __forceinline__ int unique_block_max_before(int mine, int *wave_max, int *total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl = max(incl, o);
  }
  if (lane == 63) wave_max[wave] = incl;
  __syncthreads();
  int before = __shfl_up(incl, 1, 64), all = -1;
  if (lane == 0) before = -1;
#pragma unroll
  for (int wv = 0; wv < kUniqueWaves; ++wv) {
    if (wv < wave) before = max(before, wave_max[wv]);
    all = max(all, wave_max[wv]);
  }
  *total = all;
  return before;
}

__global__ void __launch_bounds__(kUniqueThreads) gf2_unique_rekey_kernel(const u64 *P, long long ld, int wc0, int bits, long long n,
                                                                          int first, int2 *pairs) {
  const long long i = (long long)blockIdx.x * kUniqueThreads + threadIdx.x;
  if (i >= n) return;
  const int row = first ? (int)i : pairs[i].y;
  pairs[i] = make_int2((int)gf2_row_key(P + (long long)row * ld, gf2_key_window(wc0, bits)), row);
}

// lane t takes the positions s0 + t, s0 + t + 256, ... of its run: a wave reads consecutive entries of `order`
__global__ void __launch_bounds__(kUniqueThreads) gf2_unique_heads_kernel(const u64 *P, long long ld, long long w0, long long w1, int c0,
                                                                          int c1, const int *order, long long n, int *head, int *last) {
  __shared__ int wave_max[kUniqueWaves];
  const long long s0 = (long long)blockIdx.x * kUniqueRunRows + threadIdx.x;
  int m = -1, total;
#pragma unroll
  for (int i = 0; i < kUniqueRunItems; ++i) {
    const long long s = s0 + (long long)i * kUniqueThreads;
    if (s < n) {
      const bool h = s == 0 || unique_rows_differ(P + (long long)order[s - 1] * ld, P + (long long)order[s] * ld, w0, w1, c0, c1);
      head[s] = h ? (int)s : -1;
      if (h) m = (int)s;  // the positions of a lane ascend
    }
  }
  unique_block_max_before(m, wave_max, &total);
  if (threadIdx.x == 0) last[blockIdx.x] = total;
}

// one workgroup: last[r] becomes the maximum of the values before r (-1 for r == 0)
__global__ void __launch_bounds__(kUniqueThreads) gf2_unique_carry_kernel(int *last, long long runs) {
  __shared__ int wave_max[kUniqueWaves];
  int running = -1;
  for (long long b0 = 0; b0 < runs; b0 += kUniqueThreads) {
    const long long r = b0 + threadIdx.x;
    int all;
    const int before = unique_block_max_before(r < runs ? last[r] : -1, wave_max, &all);
    if (r < runs) last[r] = max(running, before);
    running = max(running, all);
    __syncthreads();  // before the next round writes wave_max
  }
}

// lane t takes the positions s0 + 4 t, ..., s0 + 4 t + 3 of its run
__global__ void __launch_bounds__(kUniqueThreads) gf2_unique_fill_kernel(int *head, long long n, const int *carry) {
  __shared__ int wave_max[kUniqueWaves];
  const long long q0 = (long long)blockIdx.x * kUniqueRunRows + (long long)kUniqueRunItems * threadIdx.x;
  int top[kUniqueRunItems], m = -1, total;
#pragma unroll
  for (int i = 0; i < kUniqueRunItems; ++i) {
    if (q0 + i < n) m = max(m, head[q0 + i]);
    top[i] = m;
  }
  const int before = max(carry[blockIdx.x], unique_block_max_before(m, wave_max, &total));
#pragma unroll
  for (int i = 0; i < kUniqueRunItems; ++i)
    if (q0 + i < n) head[q0 + i] = max(before, top[i]);
}

// the sort is stable: the head of a class holds its lowest row
__global__ void __launch_bounds__(kUniqueThreads) gf2_unique_rep_kernel(const int *order, const int *head, long long n, int *rep, int *flags) {
  const long long s = (long long)blockIdx.x * kUniqueThreads + threadIdx.x;
  if (s >= n) return;
  const int row = order[s], lowest = order[head[s]];
  if (rep) rep[row] = lowest;
  flags[row] = row == lowest;
}

dim3 unique_grid(long long items, long long per_group) { return dim3((unsigned)((items + per_group - 1) / per_group)); }  // < 2^23

}  // namespace

extern "C" hipError_t gf2k_unique_rekey(const u64 *P, long long ld, int wc0, int bits, int nrows, int first, void *pairs, hipStream_t stream) {
  if (nrows <= 0 || bits < 1 || bits > kUniqueWindowBits) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_unique_rekey_kernel, unique_grid(nrows, kUniqueThreads), dim3(kUniqueThreads), 0, stream, P, ld, wc0, bits,
                     (long long)nrows, first, static_cast<int2 *>(pairs));
  return hipGetLastError();
}

extern "C" hipError_t gf2k_unique_heads(const u64 *P, long long ld, int nrows, int c0, int c1, const int *order, int *head, int *carry,
                                        hipStream_t stream) {
  const UniquePlan plan = unique_plan(nrows, c1, c0, c1);
  if (plan.windows < 0 || nrows <= 0) return hipErrorInvalidValue;
  const dim3 runs((unsigned)plan.runs), block(kUniqueThreads);
  hipLaunchKernelGGL(gf2_unique_heads_kernel, runs, block, 0, stream, P, ld, unique_first_word(c0, c1), unique_end_word(c0, c1), c0, c1,
                     order, (long long)nrows, head, carry);
  hipLaunchKernelGGL(gf2_unique_carry_kernel, dim3(1), block, 0, stream, carry, plan.runs);
  hipLaunchKernelGGL(gf2_unique_fill_kernel, runs, block, 0, stream, head, (long long)nrows, (const int *)carry);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_unique_rep(const int *order, const int *head, int nrows, int *rep, int *flags, hipStream_t stream) {
  if (nrows <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_unique_rep_kernel, unique_grid(nrows, kUniqueThreads), dim3(kUniqueThreads), 0, stream, order, head,
                     (long long)nrows, rep, flags);
  return hipGetLastError();
}
