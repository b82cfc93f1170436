// gf2_join_rows.hip -- the kernels that turn the hash table of find/gf2_find.hip and the passes of the class sort into a grouping of a
// pool by class and a join of two pools on a column range of any width (include/m4ri_hip_join_rows.h; host side and contract:
// join_rows_host.cpp; plan and index arithmetic: join_rows_plan.h).
//
//   grouping of B (rep = the lookup of B in its own table, gf2k_find_rows):
//     pairs[j] = (the window's bits of rep[j], j)                              gf2_join_rows_pairs_kernel
//     the passes of the class sort on those pairs                              gf2k_lf2_sort_pass (lf2/gf2_lf2.hip), the last into order
//     start[r] = s where order[s] == r == rep[r]                               gf2_join_rows_starts_kernel
//     head[s] = start[rep[order[s]]]                                           gf2_join_rows_heads_kernel
//   join (idx, mult = the lookup of A in the table of B):
//     the sum of mult per run of rows of A                                     gf2_join_rows_sums_kernel
//     run sums -> run offsets, *count                                          gf2_join_rows_scan_kernel
//     offs[i] = the outputs of the rows before row i                           gf2_join_rows_offsets_kernel
//     D[t] = A[i] ^ B[order[start[idx[i]] + t - offs[i]]], ia, ib, wt          gf2_join_rows_scatter_kernel<1 | 2 | 8 | 64 lanes per row>
//
// The stable sort by rep leaves the rows of a class together and ascending, and the classes by their lowest row; the lowest row of a
// class is its rep, so it stands first, and start[] has one writer per word.  Only the words start[r] with rep[r] == r are written,
// and only those are read: idx[i] is such an r.
//
// The scatter's grid runs over fixed chunks of the OUTPUT: a workgroup bisects the offsets for the first and the last row of A of its
// chunk and deals the chunk's outputs to lane groups sized by the row width, so a class of any size costs every workgroup the same.
//
// Everything here is integer arithmetic with one writer per output word, no atomics and no waiting between workgroups: two runs give
// the same bits.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_join_rows.h"
#include "join_rows_plan.h"

namespace {

// ---- index arithmetic: plain values and pointers, no thread index (tests/test_join_rows_kernels_cpu.py runs this text on the CPU)

// the rows of A that own the outputs [t0, t1) of a chunk, t0 < t1 <= the outputs of all rows: *i0 the first, *len how many, the rows
// without outputs between them included.  offs: na offsets (join_rows_plan.h)
__device__ __forceinline__ void join_rows_chunk_rows(const long long *offs, long long na, long long t0, long long t1, long long *i0,
                                                     long long *len) {
  const long long first = join_rows_find_row(offs, 0, na, t0);
  *i0 = first;
  *len = join_rows_find_row(offs, first, na, t1 - 1) - first + 1;
}

// output t of a chunk whose rows are [i0, i0 + len): -> its row of A, and in *p its rank among that row's outputs.  pre: the offsets
// of those rows, pre[q] = offs[i0 + q] (a copy in LDS, or offs + i0)
__device__ __forceinline__ long long join_rows_output_row(const long long *pre, long long i0, long long len, long long t, long long *p) {
  const long long q = join_rows_find_row(pre, 0, len, t);
  *p = t - pre[q];
  return i0 + q;
}

// ---- the grouping

__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_pairs_kernel(const int *rep, long long n, int shift, int bits, int first,
                                                                               int2 *pairs) {
  const long long i = (long long)blockIdx.x * kJoinRowsThreads + threadIdx.x;
  if (i >= n) return;
  const int row = first ? (int)i : pairs[i].y;
  pairs[i] = make_int2((int)(((u32)rep[row] >> shift) & ((1u << bits) - 1)), row);
}

__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_starts_kernel(const int *order, const int *rep, long long n, int *start) {
  const long long s = (long long)blockIdx.x * kJoinRowsThreads + threadIdx.x;
  if (s >= n) return;
  const int row = order[s];
  if (rep[row] == row) start[row] = (int)s;
}

__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_heads_kernel(const int *order, const int *rep, const int *start, long long n,
                                                                               int *head) {
  const long long s = (long long)blockIdx.x * kJoinRowsThreads + threadIdx.x;
  if (s < n) head[s] = start[rep[order[s]]];
}

// ---- counts and offsets

// lane t takes the rows r0 + 4 t, ..., r0 + 4 t + 3 of its run
__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_sums_kernel(const int *mult, long long n, long long *sums) {
  __shared__ long long wave_sum[kJoinRowsWaves];
  const long long q0 = (long long)blockIdx.x * kJoinRowsRunRows + (long long)kJoinRowsRunItems * threadIdx.x;
  long long mine = 0, total;
#pragma unroll
  for (int i = 0; i < kJoinRowsRunItems; ++i)
    if (q0 + i < n) mine += mult[q0 + i];
  gf2_block_scan<long long, kJoinRowsWaves>(mine, wave_sum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: v[k] becomes the sum of the values before k, *total the sum of all
__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_scan_kernel(long long *v, long long n, long long *total) {
  __shared__ long long wave_sum[kJoinRowsWaves];
  long long running = 0;
  for (long long b0 = 0; b0 < n; b0 += kJoinRowsThreads * 4) {
    const long long k0 = b0 + 4ll * threadIdx.x;
    long long x[4], mine = 0, all;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = k0 + i < n ? v[k0 + i] : 0;
      mine += x[i];
    }
    long long before = running + gf2_block_scan<long long, kJoinRowsWaves>(mine, wave_sum, &all);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (k0 + i < n) v[k0 + i] = before;
      before += x[i];
    }
    running += all;
    __syncthreads();  // before the next round writes wave_sum
  }
  if (threadIdx.x == 0) *total = running;
}

__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_offsets_kernel(const int *mult, long long n, const long long *sums,
                                                                                 long long *offs) {
  __shared__ long long wave_sum[kJoinRowsWaves];
  const long long q0 = (long long)blockIdx.x * kJoinRowsRunRows + (long long)kJoinRowsRunItems * threadIdx.x;
  long long x[kJoinRowsRunItems], mine = 0, total;
#pragma unroll
  for (int i = 0; i < kJoinRowsRunItems; ++i) {
    x[i] = q0 + i < n ? mult[q0 + i] : 0;
    mine += x[i];
  }
  long long before = sums[blockIdx.x] + gf2_block_scan<long long, kJoinRowsWaves>(mine, wave_sum, &total);
#pragma unroll
  for (int i = 0; i < kJoinRowsRunItems; ++i) {
    if (q0 + i < n) offs[q0 + i] = before;
    before += x[i];
  }
}

// ---- the scatter

// d = a ^ p over the nw words of a row, the last one masked; lane `sub` of LANES takes the pairs of words sub, sub + LANES, ...
// -> the ones of this lane's words of d in the columns [wc0, wc1).  vec_a / vec_b / vec_d: see gf2_load2; an odd last word goes alone.
// (gf2_join.hip's join_xor_row, which lives in that file's unnamed namespace)
template <int LANES>
__device__ __forceinline__ int join_rows_xor_row(u64 *d, const u64 *a, const u64 *p, long long nw, u64 mlast, int vec_a, int vec_b, int vec_d,
                                                 int sub, int wc0, int wc1) {
  const long long units = (nw + 1) >> 1;
  int w = 0;
#pragma unroll 2
  for (long long u = sub; u < units; u += LANES) {
    const long long k = 2 * u;
    if (k + 1 < nw) {
      u64 x0, x1, y0, y1;
      gf2_load2(a, k, vec_a, x0, x1);
      gf2_load2(p, k, vec_b, y0, y1);
      x0 ^= y0;
      x1 ^= y1;
      if (k + 1 == nw - 1) x1 &= mlast;
      w += gf2_word_weight(x0, k, wc0, wc1) + gf2_word_weight(x1, k + 1, wc0, wc1);
      if (vec_d) {
        *reinterpret_cast<uint4 *>(d + k) = make_uint4((u32)x0, (u32)(x0 >> 32), (u32)x1, (u32)(x1 >> 32));
      } else {
        d[k] = x0;
        d[k + 1] = x1;
      }
    } else {
      const u64 x = (a[k] ^ p[k]) & mlast;
      w += gf2_word_weight(x, k, wc0, wc1);
      d[k] = x;
    }
  }
  return w;
}

// the same ones where the row is not stored: only the pairs of words that meet the weight range are read (none for an empty range)
template <int LANES>
__device__ __forceinline__ int join_rows_pair_weight(const u64 *a, const u64 *p, long long nw, int vec_a, int vec_b, int sub, int wc0, int wc1) {
  if (wc0 >= wc1) return 0;
  const long long u1 = (((long long)(wc1 - 1) >> 6) + 2) >> 1;
  int w = 0;
  for (long long u = ((long long)(wc0 >> 6) >> 1) + sub; u < u1; u += LANES) {
    const long long k = 2 * u;
    if (k + 1 < nw) {
      u64 x0, x1, y0, y1;
      gf2_load2(a, k, vec_a, x0, x1);
      gf2_load2(p, k, vec_b, y0, y1);
      w += gf2_word_weight(x0 ^ y0, k, wc0, wc1) + gf2_word_weight(x1 ^ y1, k + 1, wc0, wc1);
    } else {
      w += gf2_word_weight(a[k] ^ p[k], k, wc0, wc1);
    }
  }
  return w;
}

// Workgroup c owns the outputs [c * kJoinRowsChunk, ...) below limit = min(*count, cap); one behind the limit leaves before it reads
// an offset.  Lane 0 bisects the offsets for the chunk's rows of A; where they are at most kJoinRowsChunk their offsets are staged in
// LDS, else every output bisects offs between the chunk's ends.  The outputs are dealt to groups of LANES lanes, so the lanes of a
// wave write consecutive rows of D whatever the sizes of the classes are.  D null: the rows are not stored
template <int LANES>
__global__ void __launch_bounds__(kJoinRowsThreads) gf2_join_rows_scatter_kernel(const u64 *A, long long lda, long long na, const u64 *B,
                                                                                 long long ldb, int ncols, const int *idx, const long long *offs,
                                                                                 const int *order_b, const int *start, const long long *count,
                                                                                 u64 *D, long long ldd, long long cap, int *ia, int *ib, int *wt,
                                                                                 int wc0, int wc1, int vec_a, int vec_b, int vec_d) {
  __shared__ long long stage[kJoinRowsChunk];
  __shared__ long long ends[2];
  const long long total = *count, limit = total < cap ? total : cap;
  long long t0, t1;
  if (!join_rows_chunk_outputs(blockIdx.x, limit, &t0, &t1)) return;  // the same in every lane
  if (threadIdx.x == 0) join_rows_chunk_rows(offs, na, t0, t1, &ends[0], &ends[1]);
  __syncthreads();
  const long long i0 = ends[0], len = ends[1];
  const bool staged = len <= kJoinRowsChunk;  // the same in every lane
  if (staged)
    for (long long q = threadIdx.x; q < len; q += kJoinRowsThreads) stage[q] = offs[i0 + q];
  __syncthreads();
  const long long *pre = staged ? stage : offs + i0;
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const int sub = threadIdx.x % LANES;
  for (long long t = t0 + threadIdx.x / LANES; t < t1; t += kJoinRowsThreads / LANES) {  // the lanes of a group share t: they leave together
    long long p;
    const long long i = join_rows_output_row(pre, i0, len, t, &p);
    const int j = order_b[start[idx[i]] + p];
    const u64 *a = A + i * lda, *b = B + (long long)j * ldb;
    int w = 0;
    if (D)
      w = join_rows_xor_row<LANES>(D + t * ldd, a, b, nw, mlast, vec_a, vec_b, vec_d, sub, wc0, wc1);
    else if (wt)
      w = join_rows_pair_weight<LANES>(a, b, nw, vec_a, vec_b, sub, wc0, wc1);
#pragma unroll
    for (int d = LANES >> 1; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);  // over the lane group
    if (sub == 0) {
      if (ia) ia[t] = (int)i;
      if (ib) ib[t] = j;
      if (wt) wt[t] = w;
    }
  }
}

dim3 join_rows_grid(long long items, long long per_group) { return dim3((unsigned)((items + per_group - 1) / per_group)); }  // < 2^23

}  // namespace

extern "C" hipError_t gf2k_join_rows_pairs(const int *rep, int nrows, int shift, int bits, int first, void *pairs, hipStream_t stream) {
  if (nrows <= 0 || shift < 0 || bits < 1 || bits > kLf2MaxB || shift + bits > 31) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_join_rows_pairs_kernel, join_rows_grid(nrows, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, stream, rep,
                     (long long)nrows, shift, bits, first, static_cast<int2 *>(pairs));
  return hipGetLastError();
}

extern "C" hipError_t gf2k_join_rows_starts(const int *order, const int *rep, int nrows, int *start, hipStream_t stream) {
  if (nrows <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_join_rows_starts_kernel, join_rows_grid(nrows, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, stream, order, rep,
                     (long long)nrows, start);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_join_rows_heads(const int *order, const int *rep, const int *start, int nrows, int *head, hipStream_t stream) {
  if (nrows <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_join_rows_heads_kernel, join_rows_grid(nrows, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, stream, order, rep,
                     start, (long long)nrows, head);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_join_rows_count(const int *mult, int nrows_a, long long *sums, long long *count, hipStream_t stream) {
  if (nrows_a <= 0) return hipErrorInvalidValue;
  const long long runs = ((long long)nrows_a + kJoinRowsRunRows - 1) / kJoinRowsRunRows;
  hipLaunchKernelGGL(gf2_join_rows_sums_kernel, dim3((unsigned)runs), dim3(kJoinRowsThreads), 0, stream, mult, (long long)nrows_a, sums);
  hipLaunchKernelGGL(gf2_join_rows_scan_kernel, dim3(1), dim3(kJoinRowsThreads), 0, stream, sums, runs, count);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_join_rows_offsets(const int *mult, int nrows_a, const long long *sums, long long *offs, hipStream_t stream) {
  if (nrows_a <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_join_rows_offsets_kernel, join_rows_grid(nrows_a, kJoinRowsRunRows), dim3(kJoinRowsThreads), 0, stream, mult,
                     (long long)nrows_a, sums, offs);
  return hipGetLastError();
}

#define JOIN_ROWS_SCATTER(LANES)                                                                                                          \
  hipLaunchKernelGGL((gf2_join_rows_scatter_kernel<LANES>), grid, block, 0, stream, A, lda, (long long)nrows_a, B, ldb, ncols, idx, offs, \
                     order_b, start, count, D, ldd, (long long)cap, ia, ib, wt, wc0, wc1, vec_a, vec_b, vec_d)

extern "C" hipError_t gf2k_join_rows_scatter(const u64 *A, long long lda, int nrows_a, const u64 *B, long long ldb, int nrows_b, int ncols,
                                             const int *idx, const long long *offs, const int *order_b, const int *start, const long long *count,
                                             u64 *D, long long ldd, int cap, int *ia, int *ib, int *wt, int wc0, int wc1, int lanes,
                                             hipStream_t stream) {
  const JoinRowsPlan plan = join_rows_plan(nrows_a, nrows_b, ncols, 0, 0);
  if (plan.passes < 0 || nrows_a <= 0 || nrows_b <= 0 || cap <= 0) return hipErrorInvalidValue;
  if (lanes < 0) lanes = plan.lanes;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_a = gf2_rows_aligned16(A, lda, nrows_a, nw), vec_b = gf2_rows_aligned16(B, ldb, nrows_b, nw),
            vec_d = D ? gf2_rows_aligned16(D, ldd, cap, nw) : 0;
  const dim3 grid = join_rows_grid(cap, kJoinRowsChunk), block(kJoinRowsThreads);
  if (lanes == 1)
    JOIN_ROWS_SCATTER(1);
  else if (lanes == 2)
    JOIN_ROWS_SCATTER(2);
  else if (lanes == 8)
    JOIN_ROWS_SCATTER(8);
  else if (lanes == 64)
    JOIN_ROWS_SCATTER(64);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
