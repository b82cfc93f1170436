// gf2_draw.hip -- the draws of a randomised solver on the device (include/m4ri_hip_draw.h; host side and contract: draw_host.cpp;
// plan: draw_plan.h; the generator and every per-word rule: philox.h).
//
//   Bernoulli noise, one lane per output word (two where rows allow 16-byte stores)   gf2_bernoulli_kernel<1 | 2>
//   indices with replacement, one lane per pair of draws                              gf2_draw_indices_kernel
//   batches of k distinct values, rejection replayed in (round, position) order       gf2_draw_subsets_kernel<wave | workgroup>
//   the (key, i) pairs of a permutation; the class sort of lf2/ orders them           gf2_draw_perm_pairs_kernel
//
// A value is a function of (seed, position) alone -- a counter-based generator keeps no state --, every output word has one writer,
// and the only atomic adds integers: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "draw_plan.h"
#include "gf2_draw.h"
#include "philox.h"

namespace {

// ---- Bernoulli
// thr is uniform over the launch, so the loop over the calls of draw_bernoulli_word is a scalar loop and a plane costs one
// three-input bit operation per half word.  A lane takes unit i of the flat (row, unit) space: WORDS neighbouring words of a row.
template <int WORDS>
__global__ void __launch_bounds__(kDrawThreads) gf2_bernoulli_kernel(u64 *D, long long ld, long long rows, long long w, u64 mlast, u32 thr,
                                                                      u64 seed, u64 row0, u64 fullw, u64 colw0, int accumulate) {
  const long long units = WORDS == 2 ? (w + 1) >> 1 : w;
  const long long total = rows * units;
  const bool narrow = total < (1ll << 32);  // then the division is one of 32 bits
  for (long long i = (long long)blockIdx.x * kDrawThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kDrawThreads) {
    long long r, u;
    if (units == 1) {
      r = i;
      u = 0;
    } else if (narrow) {
      const u32 q = (u32)i / (u32)units;
      r = q;
      u = (u32)i - q * (u32)units;
    } else {
      r = i / units;
      u = i - r * units;
    }
    const long long j = WORDS * u;
    const u64 widx = (row0 + (u64)r) * fullw + colw0 + (u64)j;
    u64 *d = D + r * ld + j;
    u64 x0 = draw_bernoulli_word(seed, widx, thr);
    if (j == w - 1) x0 &= mlast;
    if (WORDS == 2 && j + 1 < w) {
      u64 x1 = draw_bernoulli_word(seed, widx + 1, thr);
      if (j + 1 == w - 1) x1 &= mlast;
      uint4 *d4 = reinterpret_cast<uint4 *>(d);
      uint4 o = make_uint4((u32)x0, (u32)(x0 >> 32), (u32)x1, (u32)(x1 >> 32));
      if (accumulate) {
        const uint4 was = *d4;
        o = make_uint4(o.x ^ was.x, o.y ^ was.y, o.z ^ was.z, o.w ^ was.w);
      }
      *d4 = o;
    } else {
      if (accumulate) x0 ^= *d;
      *d = x0;
    }
  }
}

// ---- indices: lane p makes the draws 2p and 2p + 1 from one block.  vec: idx is 8-byte aligned
__global__ void __launch_bounds__(kDrawThreads) gf2_draw_indices_kernel(int *idx, long long count, u32 n, u64 seed, int vec) {
  const long long pairs = (count + 1) >> 1;
  for (long long p = (long long)blockIdx.x * kDrawThreads + threadIdx.x; p < pairs; p += (long long)gridDim.x * kDrawThreads) {
    u32 even, odd;
    draw_index_pair(seed, (u64)p, n, &even, &odd);
    const long long t = 2 * p;
    if (t + 1 < count) {
      if (vec) {
        *reinterpret_cast<int2 *>(idx + t) = make_int2((int)even, (int)odd);
      } else {
        idx[t] = (int)even;
        idx[t + 1] = (int)odd;
      }
    } else {
      idx[t] = (int)even;
    }
  }
}

// ---- subsets
// WAVE: wave `wave` of the workgroup owns subset blockIdx.x * kDrawWaves + wave, lane t its position t (k <= 64).  Else the
// workgroup owns subset blockIdx.x and lane l the positions l, l + kDrawThreads, ...  Slot t of the subset's LDS holds (the value
// position t settled with in an EARLIER round, or -1; what it drew in this round, or -1 when it had settled before).  A round:
//   every open position draws and publishes its draw                                  barrier
//   it compares itself with all k slots through broadcast reads: it settles unless a settled value, or the draw of an open
//   position below it, is the same                                                    barrier
//   the positions that settled publish their value, every wave whether it still holds an open position                       barrier
//   no wave does: the loop ends
// which is sequential rejection sampling replayed in (round, position) order.  The loop ends after max_rounds rounds at the latest.
template <bool WAVE>
__global__ void __launch_bounds__(kDrawThreads) gf2_draw_subsets_kernel(int *sub, int batch, int k, u32 n, u64 seed, int max_rounds,
                                                                         int *unfinished) {
  constexpr int PER = WAVE ? 1 : kDrawSubsetPerLane;
  constexpr int STEP = WAVE ? kDrawSubsetWaveK : kDrawThreads;
  __shared__ int2 slots[WAVE ? kDrawWaves * kDrawSubsetWaveK : kDrawSubsetMaxK];
  __shared__ int wave_open[kDrawWaves];  // does a wave still hold an open position?  Written before the round's last barrier
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long g = WAVE ? (long long)blockIdx.x * kDrawWaves + wave : (long long)blockIdx.x;
  int2 *mine = WAVE ? slots + wave * kDrawSubsetWaveK : slots;
  const int t0 = WAVE ? lane : (int)threadIdx.x;
  const bool live = g < batch;  // the last workgroup of the wave form may hold waves without a subset: they only keep the barriers
  int val[PER];
  bool open[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int t = t0 + e * STEP;
    val[e] = -1;
    open[e] = live && t < k;
    mine[t] = make_int2(-1, -1);  // every slot has one owner
  }
  int group_open = 1;  // max_rounds >= 1 and k >= 1: a round runs
  for (int a = 0; a < max_rounds; ++a) {
    int cand[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int t = t0 + e * STEP;
      cand[e] = -2;  // equals no slot
      if (open[e]) {
        cand[e] = (int)draw_subset_candidate(seed, (u64)g * (u64)k + (u64)t, (u32)a, n);
        mine[t].y = cand[e];
      }
    }
    __syncthreads();
    bool ok[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) ok[e] = open[e];
    for (int u = 0; u < k; ++u) {
      const int2 o = mine[u];  // one address per wave: a broadcast
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int t = t0 + e * STEP;
        ok[e] = ok[e] && o.x != cand[e] && !(u < t && o.y == cand[e]);
      }
    }
    __syncthreads();  // every slot has been read ...
    int left = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      if (!open[e]) continue;
      if (ok[e]) {  // ... before the settled ones change theirs
        val[e] = cand[e];
        open[e] = false;
        mine[t0 + e * STEP] = make_int2(cand[e], -1);
      } else {
        left = 1;
      }
    }
    const int mine_open = __any(left);
    if (lane == 0) wave_open[wave] = mine_open;  // the reads of the round before lie two barriers back
    __syncthreads();
    group_open = 0;
#pragma unroll
    for (int wv = 0; wv < kDrawWaves; ++wv) group_open |= wave_open[wv];
    if (!group_open) break;  // the same answer in every lane of the workgroup
  }
  int left = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int t = t0 + e * STEP;
    if (live && t < k) sub[g * k + t] = val[e];  // -1 where the position is still open
    left |= open[e];
  }
  // one count per subset with an open position: the wave's own subset, or the workgroup's (what the last round found)
  const int unsettled = WAVE ? __any(left) : group_open;
  if (unfinished && unsettled && (WAVE ? lane == 0 : threadIdx.x == 0)) atomicAdd(unfinished, 1);
}

// ---- permutation
__global__ void __launch_bounds__(kDrawThreads) gf2_draw_perm_pairs_kernel(int2 *pairs, int n, u64 seed) {
  const long long i = (long long)blockIdx.x * kDrawThreads + threadIdx.x;
  if (i < n) pairs[i] = make_int2((int)draw_perm_key(seed, (u32)i), (int)i);
}

unsigned draw_grid(long long lanes) {
  const long long g = (lanes + kDrawThreads - 1) / kDrawThreads;
  return (unsigned)(g < 1 ? 1 : g > kDrawMaxBlocks ? kDrawMaxBlocks : g);
}

}  // namespace

#define DRAW_BERNOULLI(WORDS, LANES)                                                                                                 \
  hipLaunchKernelGGL((gf2_bernoulli_kernel<WORDS>), dim3(draw_grid(LANES)), dim3(kDrawThreads), 0, stream, D, ld, (long long)rows, w, \
                     mlast, thr, seed, (u64)row0, (u64)fullw, (u64)colw0, accumulate)

extern "C" hipError_t gf2k_bernoulli(u64 *D, long long ld, int rows, int cols, u32 thr, u64 seed, long long row0, long long fullw,
                                     long long colw0, int accumulate, hipStream_t stream) {
  if (rows <= 0 || cols <= 0 || thr == 0) return hipErrorInvalidValue;
  const long long w = ((long long)cols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)cols - 1) & 63));
  const bool vec = gf2_rows_aligned16(D, ld, rows, w);
  if (vec)
    DRAW_BERNOULLI(2, (long long)rows * ((w + 1) >> 1));
  else
    DRAW_BERNOULLI(1, (long long)rows * w);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_draw_indices(int *idx, long long count, u32 n, u64 seed, hipStream_t stream) {
  if (count <= 0 || n == 0) return hipErrorInvalidValue;
  const int vec = !(reinterpret_cast<uintptr_t>(idx) & 7);
  hipLaunchKernelGGL(gf2_draw_indices_kernel, dim3(draw_grid((count + 1) >> 1)), dim3(kDrawThreads), 0, stream, idx, count, n, seed, vec);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_draw_subsets(int *sub, int batch, int k, u32 n, u64 seed, int max_rounds, int *unfinished, hipStream_t stream) {
  const DrawSubsetPlan plan = draw_subset_plan(k);
  if (plan.per_group == 0 || batch <= 0 || n == 0 || max_rounds < 1 || max_rounds > kDrawSubsetMaxRounds) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((long long)batch + plan.per_group - 1) / plan.per_group)), block(kDrawThreads);
  if (plan.per_group > 1)
    hipLaunchKernelGGL((gf2_draw_subsets_kernel<true>), grid, block, 0, stream, sub, batch, k, n, seed, max_rounds, unfinished);
  else
    hipLaunchKernelGGL((gf2_draw_subsets_kernel<false>), grid, block, 0, stream, sub, batch, k, n, seed, max_rounds, unfinished);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_draw_perm_pairs(void *pairs, int n, u64 seed, hipStream_t stream) {
  if (n <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((long long)n + kDrawThreads - 1) / kDrawThreads));
  hipLaunchKernelGGL(gf2_draw_perm_pairs_kernel, grid, dim3(kDrawThreads), 0, stream, static_cast<int2 *>(pairs), n, seed);
  return hipGetLastError();
}
