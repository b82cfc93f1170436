// gf2_lf2.hip -- the stable class sort and one LF2 round of a BKW reduction on the device (include/m4ri_hip_lf2.h; host side and
// contract: lf2_host.cpp; plan: lf2_plan.h).
//
//   sort, per pass of up to 8 key bits (a least-significant-digit radix sort of (key, row) pairs):
//     digit counts per tile, digit-major                            gf2_lf2_sort_count_kernel
//     their exclusive sums, in two levels                           gf2_lf2_scan_sums_kernel, gf2_lf2_scan_group_kernel<int>,
//                                                                   gf2_lf2_scan_apply_kernel
//     item -> scanned offset of (digit, tile) + its rank            gf2_lf2_sort_scatter_kernel
//   b == 0: order = 0, 1, 2, ...                                    gf2_lf2_iota_kernel
//   pairs, on the sorted keys:
//     r(s) = s - t(s) summed per run of sorted positions            gf2_lf2_pair_count_kernel
//     run sums -> offsets, *count                                   gf2_lf2_scan_group_kernel<long long>
//     D[offset + j] = P[order[s]] ^ P[order[p]]                     gf2_lf2_pair_scatter_kernel<1 | 2 | 8 | 64 lanes per row>
//
// The key of a row is read by gf2_row_key (gf2_dev_words.h) alone.
//
// WHICH LANE HOLDS WHICH ITEM.  Stability rests on it.  A sort tile is kLf2TileRows consecutive items of the pass's input.  Wave w of
// the workgroup owns the items [w * kLf2WaveRows, (w + 1) * kLf2WaveRows) of the tile and walks them in rounds of 64: in round j,
// lane l holds item w * kLf2WaveRows + 64 * j + l.  So inside a tile the input order is (wave, round, lane).  The place of an item
// with digit d is
//     the scanned count of (d, tile)                 every item of a smaller digit, and of digit d in an earlier tile
//   + the items of digit d in the waves before w     run[w][d] starts there: the waves' counts of the tile, summed in wave order
//   + the items of digit d in the rounds before j    run[w][d] is advanced by the last peer of every round
//   + the peers (lanes of the same digit) below l    one ballot per digit bit, then the set bits below the lane
// which is the number of items that precede it in (digit, input order): a stable pass.  Only wave w reads or writes run[w][.] in the
// rounds.  The count kernel deals a tile's items to lanes by another rule; a count does not depend on the order.
//
// Everything is integer arithmetic with one writer per output word: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_lf2.h"
#include "lf2_plan.h"

namespace {

// the first position of the class that position s0 of the sorted keys belongs to: steps of 1, 2, 4, ... back while the key is the
// same (a class of a few rows costs a few loads), then a bisection between the last two
__device__ __forceinline__ long long lf2_class_start(const int *skeys, long long s0) {
  const int v = skeys[s0];
  long long hi = s0, lo = s0, step = 1;  // skeys[hi] == v
  for (;;) {
    lo = hi - step;
    if (lo < 0) {
      lo = -1;
      break;
    }
    if (skeys[lo] != v) break;
    hi = lo;
    step <<= 1;
  }
  while (hi - lo > 1) {  // skeys[lo] != v (or lo == -1), skeys[hi] == v
    const long long mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] == v)
      hi = mid;
    else
      lo = mid;
  }
  return hi;
}

// ---- sums over a workgroup (gf2_block_scan)

// parts[k] = the sum of chunk k of v
__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_scan_sums_kernel(const int *v, long long n, int *parts) {
  __shared__ int wave_sum[kLf2Waves];
  const long long k0 = (long long)blockIdx.x * kLf2ScanChunk + (long long)kLf2ScanItems * threadIdx.x;
  int mine = 0, total;
#pragma unroll
  for (int i = 0; i < kLf2ScanItems; ++i)
    if (k0 + i < n) mine += v[k0 + i];
  gf2_block_scan<int, kLf2Waves>(mine, wave_sum, &total);
  if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

// one workgroup: v[k] becomes the sum of the values before k, *total (unless null) the sum of all
template <typename T>
__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_scan_group_kernel(T *v, long long n, T *total) {
  __shared__ T wave_sum[kLf2Waves];
  T running = 0;
  for (long long b0 = 0; b0 < n; b0 += kLf2Threads * 4) {
    const long long k0 = b0 + 4ll * threadIdx.x;
    T x[4], mine = 0, all;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = k0 + i < n ? v[k0 + i] : 0;
      mine += x[i];
    }
    T before = running + gf2_block_scan<T, kLf2Waves>(mine, wave_sum, &all);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (k0 + i < n) v[k0 + i] = before;
      before += x[i];
    }
    running += all;
    __syncthreads();  // before the next round writes wave_sum
  }
  if (total && threadIdx.x == 0) *total = running;
}

// v[k] becomes parts[chunk] + the sum of the values before k in its chunk
__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_scan_apply_kernel(int *v, long long n, const int *parts) {
  __shared__ int wave_sum[kLf2Waves];
  const long long k0 = (long long)blockIdx.x * kLf2ScanChunk + (long long)kLf2ScanItems * threadIdx.x;
  int x[kLf2ScanItems], mine = 0, total;
#pragma unroll
  for (int i = 0; i < kLf2ScanItems; ++i) {
    x[i] = k0 + i < n ? v[k0 + i] : 0;
    mine += x[i];
  }
  int before = parts[blockIdx.x] + gf2_block_scan<int, kLf2Waves>(mine, wave_sum, &total);
#pragma unroll
  for (int i = 0; i < kLf2ScanItems; ++i) {
    if (k0 + i < n) v[k0 + i] = before;
    before += x[i];
  }
}

// ---- the sort.  P non-null: the first pass, item i is (key of row i, i); else the items are in[i] = (key, row).

__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_sort_count_kernel(const u64 *P, long long ld, int c0, int b, const int2 *in,
                                                                         long long n, int shift, int bits, long long tiles, int *counts) {
  __shared__ int cnt[kLf2Digits];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const Gf2KeyWindow w = gf2_key_window(c0, b);
  const u32 dmask = (1u << bits) - 1;
  const long long base = (long long)blockIdx.x * kLf2TileRows + threadIdx.x;
#pragma unroll 4
  for (int j = 0; j < kLf2TileItems; ++j) {
    const long long i = base + (long long)j * kLf2Threads;
    if (i < n) {
      const u32 key = P ? gf2_row_key(P + i * ld, w) : (u32)in[i].x;
      atomicAdd(&cnt[(key >> shift) & dmask], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x <= dmask) counts[(long long)threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// order non-null: the last pass, which writes order[place] = row and (skeys non-null) skeys[place] = key; else out[place] = item
__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_sort_scatter_kernel(const u64 *P, long long ld, int c0, int b, const int2 *in,
                                                                           long long n, int shift, int bits, long long tiles,
                                                                           const int *offsets, int2 *out, int *order, int *skeys) {
  __shared__ int run[kLf2Waves][kLf2Digits];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Gf2KeyWindow w = gf2_key_window(c0, b);
  const u32 dmask = (1u << bits) - 1;
  const long long base = (long long)blockIdx.x * kLf2TileRows + (long long)wave * kLf2WaveRows + lane;
  u32 key[kLf2TileItems];
  int row[kLf2TileItems];
#pragma unroll
  for (int j = 0; j < kLf2TileItems; ++j) {
    const long long i = base + 64 * j;
    key[j] = 0;
    row[j] = 0;
    if (i < n) {
      if (P) {
        key[j] = gf2_row_key(P + i * ld, w);
        row[j] = (int)i;
      } else {
        const int2 v = in[i];
        key[j] = (u32)v.x;
        row[j] = v.y;
      }
    }
  }
#pragma unroll
  for (int wv = 0; wv < kLf2Waves; ++wv) run[wv][threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kLf2TileItems; ++j)
    if (base + 64 * j < n) atomicAdd(&run[wave][(key[j] >> shift) & dmask], 1);
  __syncthreads();
  {  // lane d of the workgroup: the waves' counts of digit d become the places where their items of that digit begin
    const int d = threadIdx.x;
    int at = (u32)d <= dmask ? offsets[(long long)d * tiles + blockIdx.x] : 0;
#pragma unroll
    for (int wv = 0; wv < kLf2Waves; ++wv) {
      const int c = run[wv][d];
      run[wv][d] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kLf2TileItems; ++j) {
    const bool valid = base + 64 * j < n;
    const u32 d = (key[j] >> shift) & dmask;
    u64 peers = __ballot(valid);
    for (int k = 0; k < bits; ++k) {
      const bool bit = (d >> k) & 1;
      const u64 bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const int below = __popcll(peers & ((1ull << lane) - 1));
    int place = 0;
    if (valid) place = run[wave][d] + below;
    __syncthreads();  // every peer has read the running count ...
    if (valid && below + 1 == __popcll(peers)) run[wave][d] = place + 1;  // ... before the last one advances it
    __syncthreads();
    if (valid) {
      if (order) {
        order[place] = row[j];
        if (skeys) skeys[place] = (int)key[j];
      } else {
        out[place] = make_int2((int)key[j], row[j]);
      }
    }
  }
}

__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_iota_kernel(long long n, int *order, int *skeys) {
  const long long i = (long long)blockIdx.x * kLf2Threads + threadIdx.x;
  if (i < n) {
    order[i] = (int)i;
    if (skeys) skeys[i] = 0;
  }
}

// ---- the pairs

// r[i] = s - t(s) for the positions s = s0 + kLf2RunItems * lane + i of the run that begins at s0 (0 behind the last position), where
// t(s) is the first position of the class of s: the largest head (a position whose key differs from the one before it) at or below
// s.  The run's first position is no head of its own: lane 0 looks its class's start up.  Every lane calls it; a barrier lies inside.
__device__ __forceinline__ void lf2_run_ranks(const int *skeys, long long n, long long s0, int (&r)[kLf2RunItems], int *wave_max) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long q0 = s0 + (long long)kLf2RunItems * threadIdx.x;
  int top[kLf2RunItems], m = -1;
  int prev = threadIdx.x > 0 && q0 - 1 < n ? skeys[q0 - 1] : 0;
#pragma unroll
  for (int i = 0; i < kLf2RunItems; ++i) {
    const long long s = q0 + i;
    if (s < n) {
      const int k = skeys[s];
      int head;
      if (threadIdx.x == 0 && i == 0)
        head = (int)lf2_class_start(skeys, s0);
      else
        head = k != prev ? (int)s : -1;
      prev = k;
      m = max(m, head);
    }
    top[i] = m;
  }
  int incl = m;  // the largest head in this lane or a lane before it
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl = max(incl, o);
  }
  if (lane == 63) wave_max[wave] = incl;
  __syncthreads();
  int before = __shfl_up(incl, 1, 64);
  if (lane == 0) before = -1;
#pragma unroll
  for (int wv = 0; wv < kLf2Waves; ++wv)
    if (wv < wave) before = max(before, wave_max[wv]);
#pragma unroll
  for (int i = 0; i < kLf2RunItems; ++i) {
    const long long s = q0 + i;
    r[i] = s < n ? (int)(s - max(before, top[i])) : 0;
  }
}

__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_pair_count_kernel(const int *skeys, long long n, long long *sums) {
  __shared__ int wave_max[kLf2Waves];
  __shared__ long long wave_sum[kLf2Waves];
  int r[kLf2RunItems];
  lf2_run_ranks(skeys, n, (long long)blockIdx.x * kLf2RunRows, r, wave_max);
  long long mine = 0, total;
#pragma unroll
  for (int i = 0; i < kLf2RunItems; ++i) mine += r[i];
  gf2_block_scan<long long, kLf2Waves>(mine, wave_sum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// d = a ^ p over the nw words of a row, the last one masked; lane `sub` of LANES takes the pairs of words sub, sub + LANES, ...
// vec_p / vec_d: the rows of P / of D start on 16-byte boundaries, so a pair is one 16-byte access; an odd last word goes alone
template <int LANES>
__device__ __forceinline__ void lf2_xor_row(u64 *d, const u64 *a, const u64 *p, long long nw, u64 mlast, int vec_p, int vec_d, int sub) {
  const long long units = (nw + 1) >> 1;
#pragma unroll 2
  for (long long u = sub; u < units; u += LANES) {
    const long long k = 2 * u;
    if (k + 1 < nw) {
      u64 x0, x1;
      if (vec_p) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + k);
        const uint4 y = *reinterpret_cast<const uint4 *>(p + k);
        x0 = gf2_lo_hi(x.x ^ y.x, x.y ^ y.y);
        x1 = gf2_lo_hi(x.z ^ y.z, x.w ^ y.w);
      } else {
        x0 = a[k] ^ p[k];
        x1 = a[k + 1] ^ p[k + 1];
      }
      if (k + 1 == nw - 1) x1 &= mlast;
      if (vec_d) {
        *reinterpret_cast<uint4 *>(d + k) = make_uint4((u32)x0, (u32)(x0 >> 32), (u32)x1, (u32)(x1 >> 32));
      } else {
        d[k] = x0;
        d[k + 1] = x1;
      }
    } else {
      d[k] = (a[k] ^ p[k]) & mlast;
    }
  }
}

// A run recomputes its r(s) and their sums before every position, then deals its OUTPUTS to groups of LANES lanes: output j of the
// run belongs to the position q found by bisection in the sums, and pairs position s = s0 + q with p = t(s) + (j - pre[q]).  The
// lanes of a wave so write consecutive rows of D whatever the sizes of the classes are.
template <int LANES>
__global__ void __launch_bounds__(kLf2Threads) gf2_lf2_pair_scatter_kernel(const u64 *P, long long ld, int ncols, const int *order,
                                                                           const int *skeys, long long n, const long long *offsets, u64 *D,
                                                                           long long ldd, long long cap, int *lo, int *hi, int vec_p,
                                                                           int vec_d) {
  __shared__ long long pre[kLf2RunRows];
  __shared__ int tpos[kLf2RunRows];
  __shared__ int wave_max[kLf2Waves];
  __shared__ long long wave_sum[kLf2Waves];
  const long long off = offsets[blockIdx.x];
  if (off >= cap) return;  // the whole run lies behind the capacity: nothing of it is read
  const long long s0 = (long long)blockIdx.x * kLf2RunRows;
  int r[kLf2RunItems];
  lf2_run_ranks(skeys, n, s0, r, wave_max);
  long long mine = 0, total;
#pragma unroll
  for (int i = 0; i < kLf2RunItems; ++i) mine += r[i];
  long long before = gf2_block_scan<long long, kLf2Waves>(mine, wave_sum, &total);
#pragma unroll
  for (int i = 0; i < kLf2RunItems; ++i) {
    const int q = kLf2RunItems * threadIdx.x + i;
    pre[q] = before;
    tpos[q] = (int)(s0 + q - r[i]);
    before += r[i];
  }
  __syncthreads();
  const long long jmax = total < cap - off ? total : cap - off;  // outputs at or behind the capacity are skipped before a row is read
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const int sub = threadIdx.x % LANES;
  for (long long j = threadIdx.x / LANES; j < jmax; j += kLf2Threads / LANES) {
    const int q = gf2_find_position(pre, kLf2RunRows, j);
    const long long p = tpos[q] + (j - pre[q]);
    const int a = order[s0 + q], c = order[p];
    const long long at = off + j;
    if (sub == 0) {
      if (lo) lo[at] = c;
      if (hi) hi[at] = a;
    }
    lf2_xor_row<LANES>(D + at * ldd, P + (long long)a * ld, P + (long long)c * ld, nw, mlast, vec_p, vec_d, sub);
  }
}

}  // namespace

extern "C" hipError_t gf2k_lf2_sort_pass(const u64 *P, long long ld, int c0, int b, const void *in, int nrows, int pass, int *counts,
                                         int *parts, void *out, int *order, int *skeys, hipStream_t stream) {
  const Lf2Plan plan = lf2_plan(nrows, 0, b);
  if (plan.passes < 0 || nrows <= 0 || pass < 0 || pass >= plan.passes) return hipErrorInvalidValue;
  const int shift = kLf2DigitBits * pass, bits = lf2_pass_bits(b, pass);
  const long long n = nrows, ncounts = plan.tiles << bits, nparts = (ncounts + kLf2ScanChunk - 1) / kLf2ScanChunk;
  const dim3 tiles((unsigned)plan.tiles), chunks((unsigned)nparts), block(kLf2Threads);  // tiles < 2^19, chunks < 2^16
  const int2 *items = static_cast<const int2 *>(in);
  hipLaunchKernelGGL(gf2_lf2_sort_count_kernel, tiles, block, 0, stream, P, ld, c0, b, items, n, shift, bits, plan.tiles, counts);
  hipLaunchKernelGGL(gf2_lf2_scan_sums_kernel, chunks, block, 0, stream, (const int *)counts, ncounts, parts);
  hipLaunchKernelGGL((gf2_lf2_scan_group_kernel<int>), dim3(1), block, 0, stream, parts, nparts, (int *)nullptr);
  hipLaunchKernelGGL(gf2_lf2_scan_apply_kernel, chunks, block, 0, stream, counts, ncounts, (const int *)parts);
  hipLaunchKernelGGL(gf2_lf2_sort_scatter_kernel, tiles, block, 0, stream, P, ld, c0, b, items, n, shift, bits, plan.tiles,
                     (const int *)counts, static_cast<int2 *>(out), order, skeys);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_lf2_iota(int nrows, int *order, int *skeys, hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  const dim3 grid((unsigned)(((long long)nrows + kLf2Threads - 1) / kLf2Threads));
  hipLaunchKernelGGL(gf2_lf2_iota_kernel, grid, dim3(kLf2Threads), 0, stream, (long long)nrows, order, skeys);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_lf2_pair_count(const int *skeys, int nrows, long long *sums, long long *count, hipStream_t stream) {
  const Lf2Plan plan = lf2_plan(nrows, 0, 0);
  if (plan.passes < 0 || nrows <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_lf2_pair_count_kernel, dim3((unsigned)plan.runs), dim3(kLf2Threads), 0, stream, skeys, (long long)nrows, sums);
  hipLaunchKernelGGL((gf2_lf2_scan_group_kernel<long long>), dim3(1), dim3(kLf2Threads), 0, stream, sums, plan.runs, count);
  return hipGetLastError();
}

#define LF2_SCATTER(LANES)                                                                                                              \
  hipLaunchKernelGGL((gf2_lf2_pair_scatter_kernel<LANES>), grid, block, 0, stream, P, ld, ncols, order, skeys, (long long)nrows, offsets, D, \
                     ldd, (long long)cap, lo, hi, vec_p, vec_d)

extern "C" hipError_t gf2k_lf2_pair_scatter(const u64 *P, long long ld, int nrows, int ncols, const int *order, const int *skeys,
                                            const long long *offsets, u64 *D, long long ldd, int cap, int *lo, int *hi, int lanes,
                                            hipStream_t stream) {
  const Lf2Plan plan = lf2_plan(nrows, ncols, 0);
  if (plan.passes < 0 || nrows <= 0 || cap <= 0) return hipErrorInvalidValue;
  if (lanes < 0) lanes = plan.lanes;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_p = gf2_rows_aligned16(P, ld, nrows, nw), vec_d = gf2_rows_aligned16(D, ldd, cap, nw);
  const dim3 grid((unsigned)plan.runs), block(kLf2Threads);
  if (lanes == 1)
    LF2_SCATTER(1);
  else if (lanes == 2)
    LF2_SCATTER(2);
  else if (lanes == 8)
    LF2_SCATTER(8);
  else if (lanes == 64)
    LF2_SCATTER(64);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
