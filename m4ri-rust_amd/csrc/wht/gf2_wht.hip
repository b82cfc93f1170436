// gf2_wht.hip -- the exhaustive LPN solve on the device (include/m4ri_hip_wht.h; host side and contract: wht_host.cpp; plan: wht_plan.h;
// DESIGN.md section 7.10).
//
//   tally:      f[v] = #(rows that read v, label 0) - #(..., label 1)     gf2_wht_tally_kernel<LDS histogram | global atomics>
//   transform:  F[s] = sum over v of (-1)^popcount(s & v) f[v], in place   gf2_wht_low_kernel, gf2_wht_high_kernel<1 .. 5>
//   minimum:    the smallest value and the lowest index that holds it      gf2_wht_min_partial_kernel, gf2_wht_min_fold_kernel
//
// Everything is integer arithmetic in uint32, so wrap-around is defined and a result does not depend on the order of the adds.
//
// THE TRANSFORM.  A butterfly level l replaces the pair (a, b) of elements whose indices differ in bit l alone by (a + b, a - b); the
// levels commute, so a pass may take any set of them.  Every pass reads and writes each element once, 16 bytes per lane and
// instruction, a wave's 64 lanes on 1 KiB of consecutive addresses.
//   * gf2_wht_low_kernel: a workgroup owns a tile of 4096 consecutive elements.  Lane t of the workgroup loads the vectors t, t + 256,
//     t + 512, t + 768 of the tile, so that it holds the element bits 0-1 inside a vector and 10-11 across its vectors: four levels in
//     registers.  Bits 2-7 are the lane number: six levels by cross-lane moves (quad permutes for 1 and 2, swizzles inside 32 lanes for
//     4, 8 and 16, a permute for 32), the upper lane of a pair taking partner - own.  Bits 8-9 are the wave number: the tile goes
//     through LDS once, written and read in 16-byte pieces at consecutive lane addresses (no bank conflict in either direction, so the
//     image needs no padding), and comes back with bits 8-9 across a lane's vectors.  A tile shorter than 4096 (k < 12) leaves lanes
//     and levels out; k < 2 has no 16-byte vector and is two plain loads.
//   * gf2_wht_high_kernel<B>: levels [l0, l0 + B), l0 >= 12.  A lane owns one 16-byte column of 2^B rows that lie 2^l0 elements
//     apart and butterflies across the rows in registers; the 64 lanes of a wave read 1 KiB of each row.
// The last pass of gf2_lpn_errors_dev stores (n - F) / 2 in place of F (`fold`): no pass of its own.
#include <hip/hip_runtime.h>

#include "../gf2_kernels.h"
#include "gf2_wht.h"
#include "wht_plan.h"

typedef uint64_t u64;
typedef uint32_t u32;

namespace {

// ---- tally

// Rows by a grid-stride loop, a lane per row.  The index is bits [c0, c0 + k) of the row: one word, or two funnelled together when
// the range crosses a word boundary (k <= 30: never three); the second word is read only then, and no word at all for k == 0.
// The rule of gf2_row_key (gf2_dev_words.h) written out, not a call of it: with the call the LDS kernel compiles to other code.
template <bool LDS>
__global__ void __launch_bounds__(kWhtTallyThreads) gf2_wht_tally_kernel(const u64 *P, long long ld, long long nrows, int c0, int k,
                                                                         int label_col, u32 *f) {
  extern __shared__ u32 wht_hist[];
  const u32 size = 1u << k;
  if (LDS) {
    for (u32 i = threadIdx.x; i < size; i += kWhtTallyThreads) wht_hist[i] = 0;
    __syncthreads();
  }
  const int w0 = c0 >> 6, s = c0 & 63;
  const bool two = s + k > 64;  // then s > 0
  const u32 mask = size - 1;
  const int lw = label_col >> 6, ls = label_col & 63;
  for (long long r = (long long)blockIdx.x * kWhtTallyThreads + threadIdx.x; r < nrows; r += (long long)gridDim.x * kWhtTallyThreads) {
    const u64 *row = P + r * ld;
    u32 v = 0;
    if (k > 0) {
      u64 x = row[w0] >> s;
      if (two) x |= row[w0 + 1] << (64 - s);
      v = (u32)x & mask;
    }
    u32 d = 1u;
    if (label_col >= 0 && ((row[lw] >> ls) & 1)) d = ~0u;  // - 1
    if (LDS)
      atomicAdd(&wht_hist[v], d);
    else
      atomicAdd(&f[v], d);
  }
  if (LDS) {
    __syncthreads();
    for (u32 i = threadIdx.x; i < size; i += kWhtTallyThreads) {
      const u32 c = wht_hist[i];
      if (c) atomicAdd(&f[i], c);  // f was cleared by this call, on this stream
    }
  }
}

// ---- transform

__device__ __forceinline__ void wht_bf(u32 &a, u32 &b) {
  const u32 s = a + b, d = a - b;
  a = s;
  b = d;
}
__device__ __forceinline__ void wht_bf4(uint4 &a, uint4 &b) {
  wht_bf(a.x, b.x);
  wht_bf(a.y, b.y);
  wht_bf(a.z, b.z);
  wht_bf(a.w, b.w);
}
// levels 0 and 1, inside a vector
__device__ __forceinline__ void wht_vec(uint4 &v) {
  wht_bf(v.x, v.y);
  wht_bf(v.z, v.w);
  wht_bf(v.x, v.z);
  wht_bf(v.y, v.w);
}
__device__ __forceinline__ u32 wht_out(u32 v, int fold, u32 n) { return fold ? (n - v) >> 1 : v; }
__device__ __forceinline__ uint4 wht_out4(uint4 v, int fold, u32 n) {
  return make_uint4(wht_out(v.x, fold, n), wht_out(v.y, fold, n), wht_out(v.z, fold, n), wht_out(v.w, fold, n));
}

// the value that lane (own lane ^ M) holds
template <int M>
__device__ __forceinline__ u32 wht_from_lane_xor(u32 v) {
  if (M == 1) return (u32)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]
  if (M == 2) return (u32)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);  // quad_perm [2, 3, 0, 1]
  if (M < 32) return (u32)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (M << 10));   // bit mode: and 0x1F, or 0, xor M
  return (u32)__shfl_xor((int)v, 32, 64);
}
// one level across lanes: the lane with bit M clear takes own + partner, the other partner - own
template <int M>
__device__ __forceinline__ void wht_lane_bf(u32 &v, bool upper) {
  const u32 p = wht_from_lane_xor<M>(v);
  v = upper ? p - v : v + p;
}
template <int M>
__device__ __forceinline__ void wht_lane_level(uint4 (&x)[4], int lane) {
  const bool upper = lane & M;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wht_lane_bf<M>(x[j].x, upper);
    wht_lane_bf<M>(x[j].y, upper);
    wht_lane_bf<M>(x[j].z, upper);
    wht_lane_bf<M>(x[j].w, upper);
  }
}

// the levels [0, levels) of a tile of 2^levels elements; levels == kWhtLowLevels unless the grid is one workgroup
__global__ void __launch_bounds__(kWhtThreads) gf2_wht_low_kernel(u32 *f, int levels, int fold, u32 n) {
  __shared__ uint4 wht_tile[kWhtLdsBytes / 16];
  const int t = threadIdx.x;
  u32 *base = f + ((size_t)blockIdx.x << kWhtLowLevels);
  if (levels < 2) {  // one or two elements: no 16-byte vector (one: only the fold of gf2_lpn_errors_dev comes here)
    if (t == 0) {
      u32 a = base[0], b = levels ? base[1] : 0u;
      if (levels) wht_bf(a, b);
      base[0] = wht_out(a, fold, n);
      if (levels) base[1] = wht_out(b, fold, n);
    }
    return;
  }
  uint4 *tile = reinterpret_cast<uint4 *>(base);
  const int nvec = 1 << (levels - 2);
  uint4 x[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = j * kWhtThreads + t;
    x[j] = i < nvec ? tile[i] : make_uint4(0, 0, 0, 0);
    wht_vec(x[j]);
  }
  // element bits 2 .. 7 = lane bits 0 .. 5.  The conditions are uniform over the workgroup
  const int lane = t & 63;
  if (levels > 2) wht_lane_level<1>(x, lane);
  if (levels > 3) wht_lane_level<2>(x, lane);
  if (levels > 4) wht_lane_level<4>(x, lane);
  if (levels > 5) wht_lane_level<8>(x, lane);
  if (levels > 6) wht_lane_level<16>(x, lane);
  if (levels > 7) wht_lane_level<32>(x, lane);
  // element bits 10, 11 = vector index j
  if (levels > 10) {
    wht_bf4(x[0], x[1]);
    wht_bf4(x[2], x[3]);
  }
  if (levels > 11) {
    wht_bf4(x[0], x[2]);
    wht_bf4(x[1], x[3]);
  }
  if (levels <= 8) {  // one wave's worth of levels: nothing to exchange
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = j * kWhtThreads + t;
      if (i < nvec) tile[i] = wht_out4(x[j], fold, n);
    }
    return;
  }
  // element bits 8, 9 = wave number: through LDS, back with those bits across the lane's vectors (vector index bits 6, 7)
#pragma unroll
  for (int j = 0; j < 4; ++j) wht_tile[j * kWhtThreads + t] = x[j];
  __syncthreads();
  const int i0 = lane | ((t >> 6) << 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = wht_tile[i0 | (j << 6)];
  wht_bf4(x[0], x[1]);
  wht_bf4(x[2], x[3]);
  if (levels > 9) {
    wht_bf4(x[0], x[2]);
    wht_bf4(x[1], x[3]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 | (j << 6);
    if (i < nvec) tile[i] = wht_out4(x[j], fold, n);
  }
}

// levels [l0, l0 + B): item g = (hi, lo) is the 16-byte column lo of the 2^B rows of group hi; lv = l0 - 2 = log2 of a row's vectors
template <int B>
__global__ void __launch_bounds__(kWhtThreads) gf2_wht_high_kernel(u32 *f, int lv, long long items, int fold, u32 n) {
  constexpr int R = 1 << B;
  const long long g = (long long)blockIdx.x * kWhtThreads + threadIdx.x;
  if (g >= items) return;
  const long long hi = g >> lv, lo = g & ((1ll << lv) - 1), stride = 1ll << lv;
  uint4 *p = reinterpret_cast<uint4 *>(f) + (hi << (lv + B)) + lo;
  uint4 x[R];
#pragma unroll
  for (int r = 0; r < R; ++r) x[r] = p[r * stride];
#pragma unroll
  for (int h = 1; h < R; h <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (!(r & h)) wht_bf4(x[r], x[r | h]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) p[r * stride] = wht_out4(x[r], fold, n);
}

// ---- minimum: pairs (value, index), ordered by value, then by index, so the result does not depend on how the work is cut

struct WhtMin {
  int v, i;
};
__device__ __forceinline__ WhtMin wht_less(WhtMin a, WhtMin b) { return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// the least pair over the workgroup, valid in thread 0; every thread calls it
__device__ __forceinline__ WhtMin wht_min_block(WhtMin m, WhtMin *lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    WhtMin o;
    o.v = __shfl_xor(m.v, d, 64);
    o.i = __shfl_xor(m.i, d, 64);
    m = wht_less(m, o);
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kWhtThreads / 64; ++w) m = wht_less(m, lds[w]);
  return m;
}

// vec: w lies on a 16-byte boundary; then a lane takes four values per load and the up to three values behind the last whole vector
// go one per lane
__global__ void __launch_bounds__(kWhtThreads) gf2_wht_min_partial_kernel(const int *w, long long n, int vec, int2 *partial) {
  __shared__ WhtMin lds[kWhtThreads / 64];
  WhtMin m = {0x7FFFFFFF, 0x7FFFFFFF};  // above every pair of the array: indices end at 2^31 - 2
  const long long first = (long long)blockIdx.x * kWhtThreads + threadIdx.x, step = (long long)gridDim.x * kWhtThreads;
  long long done = 0;
  if (vec) {
    const long long nv = n >> 2;
    for (long long i = first; i < nv; i += step) {
      const int4 q = reinterpret_cast<const int4 *>(w)[i];
      const int b = (int)(4 * i);
      const WhtMin o0 = {q.x, b}, o1 = {q.y, b + 1}, o2 = {q.z, b + 2}, o3 = {q.w, b + 3};
      m = wht_less(wht_less(m, o0), wht_less(wht_less(o1, o2), o3));
    }
    done = 4 * nv;
  }
  for (long long i = done + first; i < n; i += step) {
    const WhtMin o = {w[i], (int)i};
    m = wht_less(m, o);
  }
  m = wht_min_block(m, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = make_int2(m.v, m.i);
}

// one workgroup: the least of the `count` partial pairs, all written by the launch before
__global__ void __launch_bounds__(kWhtThreads) gf2_wht_min_fold_kernel(const int2 *partial, int count, int *idx, int *val) {
  __shared__ WhtMin lds[kWhtThreads / 64];
  WhtMin m = {0x7FFFFFFF, 0x7FFFFFFF};
  for (int i = threadIdx.x; i < count; i += kWhtThreads) {
    const int2 q = partial[i];
    const WhtMin o = {q.x, q.y};
    m = wht_less(m, o);
  }
  m = wht_min_block(m, lds);
  if (threadIdx.x == 0) {
    *val = m.v;
    *idx = m.i;
  }
}

hipError_t wht_launch_pass(u32 *f, int k, const WhtPlan &plan, int p, int fold, u32 n, hipStream_t stream) {
  const int l0 = plan.first[p], b = plan.first[p + 1] - l0;
  if (p == 0) {
    const unsigned groups = 1u << (k - b);  // b == min(k, 12)
    hipLaunchKernelGGL(gf2_wht_low_kernel, dim3(groups), dim3(kWhtThreads), 0, stream, f, b, fold, n);
    return hipGetLastError();
  }
  const long long items = 1ll << (k - b - 2);  // a multiple of 256: l0 >= 12
  const dim3 grid((unsigned)(items / kWhtThreads)), block(kWhtThreads);
  switch (b) {
    case 1: hipLaunchKernelGGL((gf2_wht_high_kernel<1>), grid, block, 0, stream, f, l0 - 2, items, fold, n); break;
    case 2: hipLaunchKernelGGL((gf2_wht_high_kernel<2>), grid, block, 0, stream, f, l0 - 2, items, fold, n); break;
    case 3: hipLaunchKernelGGL((gf2_wht_high_kernel<3>), grid, block, 0, stream, f, l0 - 2, items, fold, n); break;
    case 4: hipLaunchKernelGGL((gf2_wht_high_kernel<4>), grid, block, 0, stream, f, l0 - 2, items, fold, n); break;
    case 5: hipLaunchKernelGGL((gf2_wht_high_kernel<5>), grid, block, 0, stream, f, l0 - 2, items, fold, n); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t gf2k_wht_tally(const u64 *P, long long ld, int nrows, int c0, int k, int label_col, unsigned *f, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  const dim3 grid((unsigned)wht_tally_groups(nrows, k));
  if (wht_tally_variant(k) == 0)
    hipLaunchKernelGGL((gf2_wht_tally_kernel<true>), grid, dim3(kWhtTallyThreads), sizeof(u32) << k, stream, P, ld, (long long)nrows, c0, k,
                       label_col, f);
  else
    hipLaunchKernelGGL((gf2_wht_tally_kernel<false>), grid, dim3(kWhtTallyThreads), 0, stream, P, ld, (long long)nrows, c0, k, label_col, f);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_wht_pass(unsigned *f, int k, int p, int fold, unsigned n, hipStream_t stream) {
  const WhtPlan plan = wht_plan(k);
  if (p < 0 || p >= plan.passes) return hipErrorInvalidValue;
  return wht_launch_pass(f, k, plan, p, fold, n, stream);
}

extern "C" hipError_t gf2k_wht_transform(unsigned *f, int k, int fold, unsigned n, hipStream_t stream) {
  const WhtPlan plan = wht_plan(k);
  if (plan.passes < 0) return hipErrorInvalidValue;
  if (plan.passes == 0 && fold) {  // k == 0: the identity, then (n - F) / 2 of the one element
    hipLaunchKernelGGL(gf2_wht_low_kernel, dim3(1), dim3(kWhtThreads), 0, stream, f, 0, 1, n);
    return hipGetLastError();
  }
  for (int p = 0; p < plan.passes; ++p) {
    const hipError_t e = wht_launch_pass(f, k, plan, p, fold && p == plan.passes - 1, n, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" hipError_t gf2k_wht_min(const int *w, int n, int *idx, int *val, int *partial, hipStream_t stream) {
  if (n <= 0 || !partial) return hipErrorInvalidValue;
  const int groups = (int)wht_min_groups(n);
  int2 *pairs = reinterpret_cast<int2 *>(partial);
  const int vec = !(reinterpret_cast<uintptr_t>(w) & 15);
  hipLaunchKernelGGL(gf2_wht_min_partial_kernel, dim3((unsigned)groups), dim3(kWhtThreads), 0, stream, w, (long long)n, vec, pairs);
  hipLaunchKernelGGL(gf2_wht_min_fold_kernel, dim3(1), dim3(kWhtThreads), 0, stream, pairs, groups, idx, val);
  return hipGetLastError();
}
