// gf2_weight.hip -- Hamming weights of a device matrix (include/m4ri_hip_weight.h; host side and contract: weight_host.cpp; plan:
// weight_plan.h).
//
//   rows:     weights[i] = popcount of row i                gf2_weight_rows_narrow_kernel (a lane per row; a word-level kernel)
//                                                           gf2_weight_rows_wide_kernel<8 | 64> (lanes per row, folded by __shfl_xor)
//   columns:  weights[j] = rows with bit j set              gf2_weight_cols_kernel<vec>, gf2_weight_fold_kernel
//   total:    *total = popcount of A                        gf2_weight_total_kernel<1 | 8 | 64>, one 64-bit atomic add per workgroup
//   select:   idx = the i with lo <= weights[i] <= hi       gf2_weight_select_count / _scan / _scatter_kernel
//
// Every kernel only reads A, with 64-bit row offsets, and only words below ceil(ncols / 64) of a row; the last word of a row is
// masked to the ncols bits that count (the column kernel counts its excess bits and never stores them).  16-byte loads are used only
// where the launcher has seen that every row starts on a 16-byte boundary (`vec`), and never across the end of a row's words: an odd
// last word is loaded alone.
//
// THE COLUMN KERNEL.  grid = (column groups, bands); a workgroup is wx x wy lanes: lane (x, y) owns the two word columns of slice
// group * wx + x and takes the rows band0 + y, band0 + y + wy, ... of its band, so one load instruction of a wave covers 64 / wx
// consecutive rows, 16 wx bytes of each.  Eight rows go through a carry-save tree (seven full adders of three words; sum = a ^ b ^ c
// and carry = majority are one v_bitop3_b32 per half word each) into the planes 1, 2, 4, and the tree's carry ripples into the planes
// 8, 16, 32.  After kWeightFlushRows rows, and at the end of the band, the lane empties its planes: bit j of the six planes is the
// count of column j, added to the workgroup's LDS counter of that column with an LDS integer atomic (the wy lanes of a slice meet
// there).  Lane t starts at bit t mod 64, so that the 64 lanes of a wave hit 64 different banks.  One barrier, and the counters go
// out with plain stores: into `weights` itself when there is one band, else into row `band` of the call's partial sums, which
// gf2_weight_fold_kernel adds up.  Every partial sum that is read has been stored by the same call; nothing is accumulated in
// global memory, so the result does not depend on how workgroups interleave.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_weight.h"
#include "weight_plan.h"

namespace {

// the set bits of the words sub, sub + LANES, ... of a row (pairs of words where vec); mlast masks word nw - 1
template <int LANES>
__device__ __forceinline__ int weight_row_partial(const u64 *a, long long nw, u64 mlast, int vec, int sub) {
  int c = 0;
  if (vec) {
    const long long units = (nw + 1) >> 1;
#pragma unroll 4
    for (long long u = sub; u < units; u += LANES) {
      const long long k = 2 * u;
      if (k + 1 < nw) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + k);
        u64 v1 = gf2_lo_hi(x.z, x.w);
        if (k + 1 == nw - 1) v1 &= mlast;
        c += __popcll(gf2_lo_hi(x.x, x.y)) + __popcll(v1);
      } else {
        c += __popcll(a[k] & mlast);
      }
    }
  } else {
#pragma unroll 4
    for (long long k = sub; k < nw; k += LANES) {
      u64 v = a[k];
      if (k == nw - 1) v &= mlast;
      c += __popcll(v);
    }
  }
  return c;
}

// One lane per row, rows with a grid-stride loop: no cross-lane work, no LDS, no barrier.  A wave reads 64 consecutive rows, which are
// contiguous in memory when ld equals the width.
__global__ void __launch_bounds__(256) gf2_weight_rows_narrow_kernel(const u64 *A, long long ld, long long nrows, int ncols, int vec,
                                                                     int *weights) {
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (long long)gridDim.x * blockDim.x)
    weights[r] = weight_row_partial<1>(A + r * ld, nw, mlast, vec, 0);
}

template <int LANES>
__device__ __forceinline__ int weight_fold_lanes(int c) {
#pragma unroll
  for (int d = LANES >> 1; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  return c;
}

// LANES lanes per row, 256 / LANES rows per workgroup and pass; the loop bounds are uniform over the workgroup, so every lane of a
// wave takes part in the fold.
template <int LANES>
__global__ void __launch_bounds__(kWeightThreads) gf2_weight_rows_wide_kernel(const u64 *A, long long ld, long long nrows, int ncols, int vec,
                                                                              int *weights) {
  constexpr int ROWS = kWeightThreads / LANES;
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const int sub = threadIdx.x % LANES, row = threadIdx.x / LANES;
  for (long long r0 = (long long)blockIdx.x * ROWS; r0 < nrows; r0 += (long long)gridDim.x * ROWS) {
    const long long r = r0 + row;
    int c = r < nrows ? weight_row_partial<LANES>(A + r * ld, nw, mlast, vec, sub) : 0;
    c = weight_fold_lanes<LANES>(c);
    if (sub == 0 && r < nrows) weights[r] = c;
  }
}

// the total: the row loop of the kernels above with a 64-bit sum per lane, folded over the wave, then over the four waves in LDS
template <int LANES>
__global__ void __launch_bounds__(kWeightThreads) gf2_weight_total_kernel(const u64 *A, long long ld, long long nrows, int ncols, int vec,
                                                                          unsigned long long *total) {
  constexpr int ROWS = kWeightThreads / LANES;
  __shared__ unsigned long long wave_sum[kWeightThreads / 64];
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const int sub = threadIdx.x % LANES, row = threadIdx.x / LANES;
  unsigned long long sum = 0;
  for (long long r = (long long)blockIdx.x * ROWS + row; r < nrows; r += (long long)gridDim.x * ROWS)
    sum += (unsigned long long)weight_row_partial<LANES>(A + r * ld, nw, mlast, vec, sub);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kWeightThreads / 64; ++w) s += wave_sum[w];
    if (s) atomicAdd(total, s);  // *total was cleared by this call, on this stream
  }
}

// a full adder on three words, l = their sum bit and h = their carry bit: one v_bitop3_b32 per half word each (truth tables with
// a = 0xF0, b = 0xCC, c = 0xAA: a ^ b ^ c = 0x96, majority = 0xE8)
__device__ __forceinline__ u64 weight_sum3(u64 a, u64 b, u64 c) {
  return gf2_lo_hi(__builtin_amdgcn_bitop3_b32((u32)a, (u32)b, (u32)c, 0x96),
                      __builtin_amdgcn_bitop3_b32((u32)(a >> 32), (u32)(b >> 32), (u32)(c >> 32), 0x96));
}
__device__ __forceinline__ u64 weight_carry3(u64 a, u64 b, u64 c) {
  return gf2_lo_hi(__builtin_amdgcn_bitop3_b32((u32)a, (u32)b, (u32)c, 0xE8),
                      __builtin_amdgcn_bitop3_b32((u32)(a >> 32), (u32)(b >> 32), (u32)(c >> 32), 0xE8));
}
#define WEIGHT_CSA(h, l, a, b, c)                  \
  do {                                             \
    const u64 a_ = (a), b_ = (b), c_ = (c);        \
    (h) = weight_carry3(a_, b_, c_);               \
    (l) = weight_sum3(a_, b_, c_);                 \
  } while (0)

struct WeightPlanes {
  u64 p[kWeightPlanes];  // p[i] bit j: bit i of the count of column j
};

// eight more rows of one word column
__device__ __forceinline__ void weight_csa8(WeightPlanes &n, const u64 (&d)[kWeightCsaRows]) {
  u64 ta, tb, fa, fb, e;
  WEIGHT_CSA(ta, n.p[0], n.p[0], d[0], d[1]);
  WEIGHT_CSA(tb, n.p[0], n.p[0], d[2], d[3]);
  WEIGHT_CSA(fa, n.p[1], n.p[1], ta, tb);
  WEIGHT_CSA(ta, n.p[0], n.p[0], d[4], d[5]);
  WEIGHT_CSA(tb, n.p[0], n.p[0], d[6], d[7]);
  WEIGHT_CSA(fb, n.p[1], n.p[1], ta, tb);
  WEIGHT_CSA(e, n.p[2], n.p[2], fa, fb);
  // + 8 e into the planes 8, 16, 32: the count stays below 64 (kWeightFlushRows), so nothing leaves the last plane
  u64 t = n.p[3] & e;
  n.p[3] ^= e;
  e = t;
  t = n.p[4] & e;
  n.p[4] ^= e;
  n.p[5] ^= t;
}

// the planes of one word column into the 64 LDS counters of that column.  The planes are rotated by `rot` first, so that the lanes of
// a wave start at different columns (different banks)
__device__ __forceinline__ void weight_flush(WeightPlanes &n, int *cnt, int rot) {
  u32 half[2][kWeightPlanes];
#pragma unroll
  for (int i = 0; i < kWeightPlanes; ++i) {
    const u64 q = (n.p[i] >> (rot & 63)) | (n.p[i] << ((64 - rot) & 63));  // bit t of q = bit (t + rot) mod 64 of the plane
    half[0][i] = (u32)q;
    half[1][i] = (u32)(q >> 32);
    n.p[i] = 0;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll 4
    for (int t = 0; t < 32; ++t) {
      u32 v = 0;
#pragma unroll
      for (int i = 0; i < kWeightPlanes; ++i) v |= ((half[h][i] >> t) & 1u) << i;
      atomicAdd(&cnt[(32 * h + t + rot) & 63], (int)v);
    }
  }
}

// The slices of the rows r, r + wy, ..., eight of them, below `end`.  Every load is unconditional, so that the eight are in flight
// together: a row at or behind `end` reads row end - 1 instead and is masked away, and so is a word the lane does not have (m0, m1;
// `second` is 1 where the lane has its second word, else 0: word 0 again).  WIDE: one 16-byte load per row, for lanes with both words
// in a matrix whose rows the launcher has seen on 16-byte boundaries.
template <bool WIDE>
__device__ __forceinline__ void weight_load_block(const u64 *a, long long ld, long long r, int wy, long long end, u64 m0, u64 m1, int second,
                                                  u64 (&d0)[kWeightCsaRows], u64 (&d1)[kWeightCsaRows]) {
#pragma unroll
  for (int i = 0; i < kWeightCsaRows; ++i) {
    const long long ri = r + (long long)i * wy;
    const bool ok = ri < end;
    const u64 *p = a + (ok ? ri : end - 1) * ld;
    u64 w0, w1;
    if (WIDE) {
      const uint4 v = *reinterpret_cast<const uint4 *>(p);
      w0 = gf2_lo_hi(v.x, v.y);
      w1 = gf2_lo_hi(v.z, v.w);
    } else {
      w0 = p[0];
      w1 = p[second];
    }
    d0[i] = ok ? w0 & m0 : 0ull;
    d1[i] = ok ? w1 & m1 : 0ull;
  }
}

// one lane's walk down its band: the rows first, first + wy, ... below `end` into the LDS counters of its two word columns
template <bool WIDE>
__device__ __forceinline__ void weight_band(const u64 *a, long long ld, long long first, int wy, long long end, u64 m0, u64 m1, int second,
                                            int *cnt, int rot) {
  WeightPlanes n0, n1;
#pragma unroll
  for (int i = 0; i < kWeightPlanes; ++i) n0.p[i] = n1.p[i] = 0;
  int since = 0;  // rows in the planes
  const long long step = (long long)kWeightCsaRows * wy;
  u64 d0[kWeightCsaRows], d1[kWeightCsaRows], e0[kWeightCsaRows], e1[kWeightCsaRows];
  weight_load_block<WIDE>(a, ld, first, wy, end, m0, m1, second, d0, d1);
  for (long long r = first; r < end; r += step) {  // this lane's next eight rows
    // the eight rows after these are requested first: their loads are in flight behind the adders and a flush
    weight_load_block<WIDE>(a, ld, r + step, wy, end, m0, m1, second, e0, e1);
    weight_csa8(n0, d0);
    weight_csa8(n1, d1);
    since += kWeightCsaRows;
    if (since == kWeightFlushRows) {
      weight_flush(n0, cnt, rot);
      weight_flush(n1, cnt + 64, rot);
      since = 0;
    }
#pragma unroll
    for (int i = 0; i < kWeightCsaRows; ++i) {
      d0[i] = e0[i];
      d1[i] = e1[i];
    }
  }
  if (since) {
    weight_flush(n0, cnt, rot);
    weight_flush(n1, cnt + 64, rot);
  }
}

// out: `weights` (one band) or the partial sums, row `band` of ncols ints.  Dynamic LDS: wx * 128 ints.
template <bool VEC>
__global__ void __launch_bounds__(kWeightColThreads) gf2_weight_cols_kernel(const u64 *A, long long ld, long long nrows, int ncols, int wx,
                                                                            long long lane_rows, int *out) {
  extern __shared__ int weight_cnt[];
  const int tid = threadIdx.x, wy = kWeightColThreads / wx;
  const int x = tid & (wx - 1), y = tid / wx;
  const long long nw = ((long long)ncols + 63) >> 6;
  const long long k0 = 2 * ((long long)blockIdx.x * wx + x);  // the slice's first word
  const bool has0 = k0 < nw, has1 = k0 + 1 < nw;
  const long long band0 = (long long)blockIdx.y * lane_rows * wy;  // < nrows: the plan has no empty band
  long long band1 = band0 + lane_rows * wy;
  if (band1 > nrows) band1 = nrows;
  for (int i = tid; i < wx * 128; i += kWeightColThreads) weight_cnt[i] = 0;
  __syncthreads();
  if (VEC && has1)
    weight_band<true>(A + k0, ld, band0 + y, wy, band1, ~0ull, ~0ull, 1, weight_cnt + 128 * x, tid);
  else if (has0)
    weight_band<false>(A + k0, ld, band0 + y, wy, band1, ~0ull, has1 ? ~0ull : 0ull, has1 ? 1 : 0, weight_cnt + 128 * x, tid);
  __syncthreads();
  int *o = out + (long long)blockIdx.y * ncols;
  const long long c0 = (long long)blockIdx.x * wx * 128;
  for (int i = tid; i < wx * 128; i += kWeightColThreads)
    if (c0 + i < ncols) o[c0 + i] = weight_cnt[i];
}

// weights[c] = sum over the bands of partial[band][c]; blockDim = (64 columns, 16 stripes of bands)
__global__ void __launch_bounds__(1024) gf2_weight_fold_kernel(const int *partial, long long bands, int ncols, int *weights) {
  __shared__ int stripe[16][64];
  const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
  int s = 0;
  if (c < ncols)
    for (long long b = threadIdx.y; b < bands; b += 16) s += partial[b * ncols + c];
  stripe[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y == 0 && c < ncols) {
#pragma unroll
    for (int i = 1; i < 16; ++i) s += stripe[i][threadIdx.x];
    weights[c] = s;
  }
}

// ---- select: ordered compaction.  A block covers kWeightSelectBlock consecutive weights, thread t the kWeightSelectItems behind
// base + kWeightSelectItems * t, so ranks within a block follow the index order.

__device__ __forceinline__ int weight_matches(const int *w, long long i0, long long n, int lo, int hi, bool (&m)[kWeightSelectItems]) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < kWeightSelectItems; ++k) {
    m[k] = false;
    if (i0 + k < n) {
      const int v = w[i0 + k];
      m[k] = lo <= v && v <= hi;
    }
    c += m[k];
  }
  return c;
}

// inclusive sums of v over the 256 threads of a workgroup (Hillis-Steele in LDS); every thread calls it
__device__ __forceinline__ int weight_block_scan(int v, int *lds, int tid) {
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < kWeightThreads; d <<= 1) {
    const int t = tid >= d ? lds[tid - d] : 0;
    __syncthreads();
    lds[tid] += t;
    __syncthreads();
  }
  return lds[tid];
}

__global__ void __launch_bounds__(kWeightThreads) gf2_weight_select_count_kernel(const int *w, long long n, int lo, int hi, int *counts) {
  __shared__ int lds[kWeightThreads];
  bool m[kWeightSelectItems];
  const int c = weight_matches(w, (long long)blockIdx.x * kWeightSelectBlock + kWeightSelectItems * threadIdx.x, n, lo, hi, m);
  const int incl = weight_block_scan(c, lds, threadIdx.x);
  if (threadIdx.x == kWeightThreads - 1) counts[blockIdx.x] = incl;
}

// one workgroup: counts[b] becomes the number of matches in the blocks before b, *count the number of all
__global__ void __launch_bounds__(kWeightThreads) gf2_weight_select_scan_kernel(int *counts, long long nblk, int *count) {
  __shared__ int lds[kWeightThreads];
  int running = 0;
  for (long long b0 = 0; b0 < nblk; b0 += kWeightThreads) {
    const long long b = b0 + threadIdx.x;
    const int v = b < nblk ? counts[b] : 0;
    const int incl = weight_block_scan(v, lds, threadIdx.x);
    if (b < nblk) counts[b] = running + incl - v;
    running += lds[kWeightThreads - 1];
    __syncthreads();  // before the next round writes lds
  }
  if (threadIdx.x == 0) *count = running;
}

__global__ void __launch_bounds__(kWeightThreads) gf2_weight_select_scatter_kernel(const int *w, long long n, int lo, int hi, const int *offsets,
                                                                                  int *idx, int cap) {
  __shared__ int lds[kWeightThreads];
  bool m[kWeightSelectItems];
  const long long i0 = (long long)blockIdx.x * kWeightSelectBlock + kWeightSelectItems * threadIdx.x;
  const int c = weight_matches(w, i0, n, lo, hi, m);
  const int incl = weight_block_scan(c, lds, threadIdx.x);
  long long pos = (long long)offsets[blockIdx.x] + incl - c;
#pragma unroll
  for (int k = 0; k < kWeightSelectItems; ++k)
    if (m[k]) {
      if (pos < cap) idx[pos] = (int)(i0 + k);
      ++pos;
    }
}

}  // namespace

extern "C" hipError_t gf2k_weight_rows_narrow(const u64 *A, long long ld, int nrows, int ncols, int *weights, hipStream_t stream) {
  if (nrows <= 0 || ncols <= 0) return hipSuccess;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec = gf2_rows_aligned16(A, ld, nrows, nw);
  const long long blocks = ((long long)nrows + 255) / 256;
  hipLaunchKernelGGL(gf2_weight_rows_narrow_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, stream, A, ld,
                     (long long)nrows, ncols, vec, weights);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_weight_rows(const u64 *A, long long ld, int nrows, int ncols, int *weights, hipStream_t stream) {
  if (nrows <= 0 || ncols <= 0) return hipSuccess;
  const WeightRowsPlan plan = weight_rows_plan(nrows, ncols);
  if (plan.variant == 0) return gf2k_weight_rows_narrow(A, ld, nrows, ncols, weights, stream);
  const int vec = gf2_rows_aligned16(A, ld, nrows, ((long long)ncols + 63) >> 6);
  const long long blocks = ((long long)nrows + plan.rows - 1) / plan.rows;
  const dim3 grid((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks));
  if (plan.lanes == 8)
    hipLaunchKernelGGL((gf2_weight_rows_wide_kernel<8>), grid, dim3(kWeightThreads), 0, stream, A, ld, (long long)nrows, ncols, vec, weights);
  else
    hipLaunchKernelGGL((gf2_weight_rows_wide_kernel<64>), grid, dim3(kWeightThreads), 0, stream, A, ld, (long long)nrows, ncols, vec, weights);
  return hipGetLastError();
}

// *total must have been cleared on `stream`
extern "C" hipError_t gf2k_weight_total(const u64 *A, long long ld, int nrows, int ncols, unsigned long long *total, hipStream_t stream) {
  if (nrows <= 0 || ncols <= 0) return hipSuccess;
  const WeightTotalPlan plan = weight_total_plan(nrows, ncols);
  const int vec = gf2_rows_aligned16(A, ld, nrows, ((long long)ncols + 63) >> 6);
  const long long blocks = ((long long)nrows + plan.rows - 1) / plan.rows;
  const dim3 grid((unsigned)(blocks > kWeightTotalBlocks ? kWeightTotalBlocks : blocks));
  if (plan.lanes == 1)
    hipLaunchKernelGGL((gf2_weight_total_kernel<1>), grid, dim3(kWeightThreads), 0, stream, A, ld, (long long)nrows, ncols, vec, total);
  else if (plan.lanes == 8)
    hipLaunchKernelGGL((gf2_weight_total_kernel<8>), grid, dim3(kWeightThreads), 0, stream, A, ld, (long long)nrows, ncols, vec, total);
  else
    hipLaunchKernelGGL((gf2_weight_total_kernel<64>), grid, dim3(kWeightThreads), 0, stream, A, ld, (long long)nrows, ncols, vec, total);
  return hipGetLastError();
}

// partial: weight_cols_plan(nrows, ncols).scratch bytes when the plan has more than one band, else unused
extern "C" hipError_t gf2k_weight_cols(const u64 *A, long long ld, int nrows, int ncols, int *weights, int *partial, hipStream_t stream) {
  if (nrows <= 0 || ncols <= 0) return hipSuccess;
  const WeightColsPlan plan = weight_cols_plan(nrows, ncols);
  if (plan.bands > 1 && !partial) return hipErrorInvalidValue;
  const bool vec = gf2_rows_aligned16(A, ld, nrows, ((long long)ncols + 63) >> 6);
  const dim3 grid((unsigned)plan.groups, (unsigned)plan.bands);  // groups < 2^19, bands <= 1024
  const size_t lds = sizeof(int) * 128 * (size_t)plan.wx;
  int *out = plan.bands > 1 ? partial : weights;
  if (vec)
    hipLaunchKernelGGL((gf2_weight_cols_kernel<true>), grid, dim3(kWeightColThreads), lds, stream, A, ld, (long long)nrows, ncols, plan.wx,
                       plan.lane_rows, out);
  else
    hipLaunchKernelGGL((gf2_weight_cols_kernel<false>), grid, dim3(kWeightColThreads), lds, stream, A, ld, (long long)nrows, ncols, plan.wx,
                       plan.lane_rows, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || plan.bands == 1) return e;
  hipLaunchKernelGGL(gf2_weight_fold_kernel, dim3((unsigned)(((long long)ncols + 63) / 64)), dim3(64, 16), 0, stream, partial, plan.bands, ncols,
                     weights);
  return hipGetLastError();
}

// block_counts: ceil(n / kWeightSelectBlock) ints of scratch, written here before they are read
extern "C" hipError_t gf2k_weight_select(const int *weights, int n, int lo, int hi, int *idx, int cap, int *count, int *block_counts,
                                         hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const long long nblk = ((long long)n + kWeightSelectBlock - 1) / kWeightSelectBlock;  // < 2^21
  hipLaunchKernelGGL(gf2_weight_select_count_kernel, dim3((unsigned)nblk), dim3(kWeightThreads), 0, stream, weights, (long long)n, lo, hi,
                     block_counts);
  hipLaunchKernelGGL(gf2_weight_select_scan_kernel, dim3(1), dim3(kWeightThreads), 0, stream, block_counts, nblk, count);
  if (cap > 0)
    hipLaunchKernelGGL(gf2_weight_select_scatter_kernel, dim3((unsigned)nblk), dim3(kWeightThreads), 0, stream, weights, (long long)n, lo, hi,
                       block_counts, idx, cap);
  return hipGetLastError();
}
