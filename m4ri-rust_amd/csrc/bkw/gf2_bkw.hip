// gf2_bkw.hip -- one LF1 round of a BKW reduction on the device (include/m4ri_hip_bkw.h; host side and contract: bkw_host.cpp; plan:
// bkw_plan.h).
//
//   class firsts:  first[v] = the lowest row whose key is v      gf2_lf1_first_kernel<LDS table | global atomics>
//   count:         survivors per run of rows                      gf2_lf1_count_kernel<rows per lane>
//   scan:          block counts -> offsets, *count                gf2_lf1_scan_kernel
//   scatter:       D[offset + rank] = P[i] ^ P[first[key(i)]]     gf2_lf1_scatter_kernel<1 | 2 | 8 | 64 lanes per row, rows per lane>
//
// The key of a row is read by gf2_row_key (gf2_dev_words.h) alone.  A minimum of row indices does not depend on the order in which
// the rows arrive, the ranks come from ballots and integer sums, and every row of D has one writer: the results are the same bits in
// every run.
//
// THE TABLE.  `first` is preset to all-ones bytes by the caller (a memset on the stream), which is above every row index as an
// unsigned value and reads -1 as an int: an empty class needs no pass of its own.  A table entry only ever decreases, so a row that
// reads an entry at or below its own index (a relaxed load; a stale value is only larger) has nothing to add and issues no atomic:
// with more rows than classes nearly every row stops at that load.
//
// THE RANKS.  Lane t of a workgroup takes the rows t, t + 256, ... of the workgroup's run, so a wave looks at 64 consecutive rows at
// a time: segment j * 4 + wave.  The rank of a survivor inside its segment is the number of set ballot bits below its lane; the
// segments' counts go through LDS once and every lane sums the ones before its own.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "bkw_plan.h"
#include "gf2_bkw.h"

namespace {

// ---- class firsts: rows by a grid-stride loop, a lane per row

template <bool LDS>
__global__ void __launch_bounds__(kLf1FirstThreads) gf2_lf1_first_kernel(const u64 *P, long long ld, long long nrows, int c0, int b,
                                                                         u32 *first) {
  extern __shared__ u32 lf1_table[];
  const u32 size = 1u << b;
  if (LDS) {
    for (u32 i = threadIdx.x; i < size; i += kLf1FirstThreads) lf1_table[i] = ~0u;
    __syncthreads();
  }
  const Gf2KeyWindow w = gf2_key_window(c0, b);
  for (long long r = (long long)blockIdx.x * kLf1FirstThreads + threadIdx.x; r < nrows; r += (long long)gridDim.x * kLf1FirstThreads) {
    const u32 v = gf2_row_key(P + r * ld, w);
    // the result of the atomic is not used: the no-return form
    if (LDS) {
      if (__atomic_load_n(&lf1_table[v], __ATOMIC_RELAXED) > (u32)r) atomicMin(&lf1_table[v], (u32)r);
    } else {
      if (__atomic_load_n(&first[v], __ATOMIC_RELAXED) > (u32)r) atomicMin(&first[v], (u32)r);
    }
  }
  if (LDS) {
    __syncthreads();
    for (u32 i = threadIdx.x; i < size; i += kLf1FirstThreads) {
      const u32 c = lf1_table[i];
      if (c != ~0u && __atomic_load_n(&first[i], __ATOMIC_RELAXED) > c) atomicMin(&first[i], c);
    }
  }
}

// ---- count and scatter share the survivor rule

struct Lf1Row {
  bool survives;
  int partner;  // the row to XOR in, -1: none (a kept row of key 0)
};

__device__ __forceinline__ Lf1Row lf1_row(const u64 *P, long long ld, long long r, long long nrows, Gf2KeyWindow w, int keep_zero,
                                           const int *first) {
  Lf1Row o = {false, -1};
  if (r < nrows) {
    const u32 v = gf2_row_key(P + r * ld, w);
    const int f = first[v];
    if (keep_zero && v == 0)
      o.survives = true;
    else if (f != (int)r) {
      o.survives = true;
      o.partner = f;
    }
  }
  return o;
}

// the survivors of the workgroup's run before this lane's row of pass j, and (in *total) of the whole run.  Every lane calls it.
template <int ITEMS>
__device__ __forceinline__ void lf1_ranks(const bool (&m)[ITEMS], int (&rank)[ITEMS], int *seg, int *total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64 bal[ITEMS];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    bal[j] = __ballot(m[j]);
    if (lane == 0) seg[j * (kLf1Threads / 64) + wave] = __popcll(bal[j]);
  }
  __syncthreads();
  int before = 0, k = 0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
#pragma unroll
    for (int wv = 0; wv < kLf1Threads / 64; ++wv, ++k) {
      if (wv == wave) rank[j] = before + __popcll(bal[j] & ((1ull << lane) - 1));
      before += seg[k];
    }
  }
  *total = before;
}

template <int ITEMS>
__global__ void __launch_bounds__(kLf1Threads) gf2_lf1_count_kernel(const u64 *P, long long ld, long long nrows, int c0, int b, int keep_zero,
                                                                    const int *first, int *counts) {
  __shared__ int seg[ITEMS * (kLf1Threads / 64)];
  const Gf2KeyWindow w = gf2_key_window(c0, b);
  const long long base = (long long)blockIdx.x * (kLf1Threads * ITEMS) + threadIdx.x;
  bool m[ITEMS];
  int rank[ITEMS], total;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) m[j] = lf1_row(P, ld, base + j * kLf1Threads, nrows, w, keep_zero, first).survives;
  lf1_ranks<ITEMS>(m, rank, seg, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup: counts[k] becomes the number of survivors in the blocks before k, *count the number of all.  A round takes
// kLf1ScanChunk counts, kLf1ScanItems consecutive ones per lane.
__global__ void __launch_bounds__(kLf1Threads) gf2_lf1_scan_kernel(int *counts, long long nblk, int *count) {
  __shared__ int wave_sum[kLf1Threads / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int running = 0;
  for (long long b0 = 0; b0 < nblk; b0 += kLf1ScanChunk) {
    const long long k0 = b0 + (long long)kLf1ScanItems * threadIdx.x;
    int v[kLf1ScanItems], mine = 0;
#pragma unroll
    for (int i = 0; i < kLf1ScanItems; ++i) {
      v[i] = k0 + i < nblk ? counts[k0 + i] : 0;
      mine += v[i];
    }
    // the wave scan written out, not gf2_block_scan: with the call this kernel compiles to other code (25 -> 28 VGPRs)
    int incl = mine;  // inclusive sums over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = running + incl - mine, all = 0;
#pragma unroll
    for (int wv = 0; wv < kLf1Threads / 64; ++wv) {
      if (wv < wave) before += wave_sum[wv];
      all += wave_sum[wv];
    }
#pragma unroll
    for (int i = 0; i < kLf1ScanItems; ++i) {
      if (k0 + i < nblk) counts[k0 + i] = before;
      before += v[i];
    }
    running += all;
    __syncthreads();  // before the next round writes wave_sum
  }
  if (threadIdx.x == 0) *count = running;
}

// ---- scatter

// d = a ^ p (p null: d = a) over the nw words of a row, the last one masked; lane `sub` of LANES takes the pairs of words sub,
// sub + LANES, ...  vec_p / vec_d: the rows of P / of D start on 16-byte boundaries, so a pair is one 16-byte access; an odd last word
// goes alone either way
template <int LANES>
__device__ __forceinline__ void lf1_xor_row(u64 *d, const u64 *a, const u64 *p, long long nw, u64 mlast, int vec_p, int vec_d, int sub) {
  const long long units = (nw + 1) >> 1;
#pragma unroll 2
  for (long long u = sub; u < units; u += LANES) {
    const long long k = 2 * u;
    if (k + 1 < nw) {
      u64 x0, x1;
      if (vec_p) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + k);
        x0 = gf2_lo_hi(x.x, x.y);
        x1 = gf2_lo_hi(x.z, x.w);
        if (p) {
          const uint4 y = *reinterpret_cast<const uint4 *>(p + k);
          x0 ^= gf2_lo_hi(y.x, y.y);
          x1 ^= gf2_lo_hi(y.z, y.w);
        }
      } else {
        x0 = a[k];
        x1 = a[k + 1];
        if (p) {
          x0 ^= p[k];
          x1 ^= p[k + 1];
        }
      }
      if (k + 1 == nw - 1) x1 &= mlast;
      if (vec_d) {
        *reinterpret_cast<uint4 *>(d + k) = make_uint4((u32)x0, (u32)(x0 >> 32), (u32)x1, (u32)(x1 >> 32));
      } else {
        d[k] = x0;
        d[k + 1] = x1;
      }
    } else {
      u64 x = a[k];
      if (p) x ^= p[k];
      d[k] = x & mlast;
    }
  }
}

// Every lane first ranks its own rows of the run (ITEMS of them).  LANES == 1: it then moves them itself.  LANES > 1: destination and
// partner of every row go to LDS, and LANES lanes move a row together, 256 / LANES rows per pass, a pair of words per lane and step:
// the lanes of a wave then read and write consecutive 16-byte pieces.
template <int LANES, int ITEMS>
__global__ void __launch_bounds__(kLf1Threads) gf2_lf1_scatter_kernel(const u64 *P, long long ld, long long nrows, int ncols, int c0, int b,
                                                                      int keep_zero, const int *first, const int *offsets, u64 *D,
                                                                      long long ldd, int cap, int *src, int vec_p, int vec_d) {
  constexpr int RUN = kLf1Threads * ITEMS;
  __shared__ int seg[ITEMS * (kLf1Threads / 64)];
  __shared__ int dest[LANES == 1 ? 1 : RUN], mate[LANES == 1 ? 1 : RUN];
  const Gf2KeyWindow w = gf2_key_window(c0, b);
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const long long run0 = (long long)blockIdx.x * RUN;
  Lf1Row row[ITEMS];
  bool m[ITEMS];
  int rank[ITEMS], total;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    row[j] = lf1_row(P, ld, run0 + j * kLf1Threads + threadIdx.x, nrows, w, keep_zero, first);
    m[j] = row[j].survives;
  }
  lf1_ranks<ITEMS>(m, rank, seg, &total);
  const long long off = offsets[blockIdx.x];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int q = j * kLf1Threads + threadIdx.x;
    const long long r = run0 + q, pos = off + rank[j];
    const bool store = m[j] && pos < cap;
    if (store && src) src[pos] = (int)r;
    if (LANES == 1) {
      if (store)
        lf1_xor_row<1>(D + pos * ldd, P + r * ld, row[j].partner >= 0 ? P + (long long)row[j].partner * ld : nullptr, nw, mlast, vec_p, vec_d,
                       0);
    } else {
      dest[q] = store ? (int)pos : -1;
      mate[q] = row[j].partner;
    }
  }
  if (LANES > 1) {
    __syncthreads();
    const int sub = threadIdx.x % LANES;
    for (int q = threadIdx.x / LANES; q < RUN; q += kLf1Threads / LANES) {
      const int to = dest[q];
      if (to < 0) continue;
      const int f = mate[q];
      lf1_xor_row<LANES>(D + (long long)to * ldd, P + (run0 + q) * ld, f >= 0 ? P + (long long)f * ld : nullptr, nw, mlast, vec_p, vec_d, sub);
    }
  }
}

}  // namespace

extern "C" hipError_t gf2k_lf1_first(const u64 *P, long long ld, int nrows, int c0, int b, int *first, int variant, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  if (variant < 0) variant = lf1_first_variant(b);
  if (variant == 0 && b > kLf1LdsLevels) return hipErrorInvalidValue;  // the table would not fit
  const dim3 grid((unsigned)lf1_first_groups(nrows, variant));
  u32 *table = reinterpret_cast<u32 *>(first);
  if (variant == 0)
    hipLaunchKernelGGL((gf2_lf1_first_kernel<true>), grid, dim3(kLf1FirstThreads), sizeof(u32) << b, stream, P, ld, (long long)nrows, c0, b,
                       table);
  else
    hipLaunchKernelGGL((gf2_lf1_first_kernel<false>), grid, dim3(kLf1FirstThreads), 0, stream, P, ld, (long long)nrows, c0, b, table);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_lf1_count(const u64 *P, long long ld, int nrows, int ncols, int c0, int b, int keep_zero, const int *first,
                                     int *block_counts, hipStream_t stream) {
  const Lf1Plan plan = lf1_plan(nrows, ncols, b);
  if (plan.variant < 0 || nrows <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)plan.blocks), block(kLf1Threads);  // blocks < 2^23
  if (plan.rows == kLf1Threads * kLf1NarrowItems)
    hipLaunchKernelGGL((gf2_lf1_count_kernel<kLf1NarrowItems>), grid, block, 0, stream, P, ld, (long long)nrows, c0, b, keep_zero, first,
                       block_counts);
  else
    hipLaunchKernelGGL((gf2_lf1_count_kernel<1>), grid, block, 0, stream, P, ld, (long long)nrows, c0, b, keep_zero, first, block_counts);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_lf1_scan(int *block_counts, long long nblk, int *count, hipStream_t stream) {
  hipLaunchKernelGGL(gf2_lf1_scan_kernel, dim3(1), dim3(kLf1Threads), 0, stream, block_counts, nblk, count);
  return hipGetLastError();
}

#define LF1_SCATTER(LANES, ITEMS)                                                                                                       \
  hipLaunchKernelGGL((gf2_lf1_scatter_kernel<LANES, ITEMS>), grid, block, 0, stream, P, ld, (long long)nrows, ncols, c0, b, keep_zero, first, \
                     offsets, D, ldd, cap, src, vec_p, vec_d)

extern "C" hipError_t gf2k_lf1_scatter(const u64 *P, long long ld, int nrows, int ncols, int c0, int b, int keep_zero, const int *first,
                                       const int *offsets, u64 *D, long long ldd, int cap, int *src, int lanes, hipStream_t stream) {
  const Lf1Plan plan = lf1_plan(nrows, ncols, b);
  if (plan.variant < 0 || nrows <= 0 || cap <= 0) return hipErrorInvalidValue;
  const bool narrow = plan.rows == kLf1Threads * kLf1NarrowItems;
  if (lanes < 0) lanes = plan.lanes;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_p = gf2_rows_aligned16(P, ld, nrows, nw), vec_d = gf2_rows_aligned16(D, ldd, cap, nw);
  const dim3 grid((unsigned)plan.blocks), block(kLf1Threads);
  if (narrow && lanes == 1)
    LF1_SCATTER(1, kLf1NarrowItems);
  else if (narrow && lanes == 2)
    LF1_SCATTER(2, kLf1NarrowItems);
  else if (!narrow && lanes == 8)
    LF1_SCATTER(8, 1);
  else if (!narrow && lanes == 64)
    LF1_SCATTER(64, 1);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
