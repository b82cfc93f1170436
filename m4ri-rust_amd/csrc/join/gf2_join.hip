// gf2_join.hip -- the join of two pools on a window of bits, with the weights of the XORs, on the device (include/m4ri_hip_join.h; host
// side and contract: join_host.cpp; plan: join_plan.h).  A and B are sorted by the class sort of
// lf2/gf2_lf2.hip (gf2k_lf2_sort_pass); the kernels here run on the sorted keys:
//
//     u(s) - l(s), the positions of B with the key of position s of A, summed per run      gf2_join_count_kernel
//     run sums -> offsets, *count                                                           gf2_join_scan_kernel
//     D[offset + j] = A[order_a[s]] ^ B[order_b[p]], ia, ib, the weight of D[offset + j]     gf2_join_scatter_kernel<1 | 2 | 8 | 64 lanes per row>
//
// A workgroup owns a run of kJoinRunRows consecutive sorted positions of A.  It bisects the sorted keys of B once for the run's first
// key and once for its last: the SPAN of positions of B that the run can meet.  A span of at most kJoinSpanKeys keys is copied into
// LDS and every position finds its l(s) and u(s) there; a longer one (B much larger than A, or a giant class) is bisected in global
// memory between the span's ends.
//
// Everything is integer arithmetic with one writer per output word and no atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_join.h"
#include "join_plan.h"

namespace {

// ---- word-level helpers: plain pointers, no thread index (tests/test_join_helpers_cpu.py runs their text on the CPU)

// the first position p of [lo, hi) with keys[p] >= v, hi where there is none; keys ascending.  Reads keys[lo .. hi) alone
__device__ __forceinline__ long long join_lower_bound(const int *keys, long long lo, long long hi, int v) {
  while (lo < hi) {  // every position before lo holds a key < v, every one from hi on a key >= v
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// the first position p of [lo, hi) with keys[p] > v, hi where there is none
__device__ __forceinline__ long long join_upper_bound(const int *keys, long long lo, long long hi, int v) {
  while (lo < hi) {  // every position before lo holds a key <= v, every one from hi on a key > v
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- sums over a workgroup (gf2_block_scan)

// one workgroup: v[k] becomes the sum of the values before k, *total the sum of all
__global__ void __launch_bounds__(kJoinThreads) gf2_join_scan_kernel(long long *v, long long n, long long *total) {
  __shared__ long long wave_sum[kJoinWaves];
  long long running = 0;
  for (long long b0 = 0; b0 < n; b0 += kJoinThreads * 4) {
    const long long k0 = b0 + 4ll * threadIdx.x;
    long long x[4], mine = 0, all;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = k0 + i < n ? v[k0 + i] : 0;
      mine += x[i];
    }
    long long before = running + gf2_block_scan<long long, kJoinWaves>(mine, wave_sum, &all);
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

// ---- the partners of a run

// l[i] = l(s) and c[i] = u(s) - l(s) for the positions s = s0 + kJoinRunItems * lane + i of the run of A that begins at s0 (both 0
// behind the last position): [l(s), u(s)) are the positions of B's sorted keys that hold the key of s.  stage (kJoinSpanKeys ints)
// and span (2 ints) are LDS.  Every lane calls it; two barriers lie inside.
__device__ __forceinline__ void join_run_partners(const int *ska, long long na, const int *skb, long long nb, long long s0, int *stage,
                                                  int *span, int (&l)[kJoinRunItems], int (&c)[kJoinRunItems]) {
  if (threadIdx.x == 0) {
    const long long last = (s0 + kJoinRunRows < na ? s0 + kJoinRunRows : na) - 1;
    const long long b0 = join_lower_bound(skb, 0, nb, ska[s0]);
    span[0] = (int)b0;
    span[1] = (int)join_upper_bound(skb, b0, nb, ska[last]);
  }
  __syncthreads();
  const long long b0 = span[0], b1 = span[1], len = b1 - b0;
  const bool staged = len <= kJoinSpanKeys;  // the same in every lane
  if (staged)
    for (long long i = threadIdx.x; i < len; i += kJoinThreads) stage[i] = skb[b0 + i];
  __syncthreads();
  const long long q0 = s0 + (long long)kJoinRunItems * threadIdx.x;
  int prev = -1, pl = 0, pc = 0;  // a key is never negative; consecutive positions of one key share their partners
#pragma unroll
  for (int i = 0; i < kJoinRunItems; ++i) {
    const long long s = q0 + i;
    l[i] = 0;
    c[i] = 0;
    if (s < na) {
      const int k = ska[s];
      if (k != prev) {
        long long lb, ub;
        if (staged) {
          lb = join_lower_bound(stage, 0, len, k);
          ub = join_upper_bound(stage, lb, len, k);
          lb += b0;
          ub += b0;
        } else {
          lb = join_lower_bound(skb, b0, b1, k);
          ub = join_upper_bound(skb, lb, b1, k);
        }
        prev = k;
        pl = (int)lb;
        pc = (int)(ub - lb);
      }
      l[i] = pl;
      c[i] = pc;
    }
  }
}

__global__ void __launch_bounds__(kJoinThreads) gf2_join_count_kernel(const int *ska, long long na, const int *skb, long long nb,
                                                                      long long *sums) {
  __shared__ int stage[kJoinSpanKeys];
  __shared__ int span[2];
  __shared__ long long wave_sum[kJoinWaves];
  int l[kJoinRunItems], c[kJoinRunItems];
  join_run_partners(ska, na, skb, nb, (long long)blockIdx.x * kJoinRunRows, stage, span, l, c);
  long long mine = 0, total;
#pragma unroll
  for (int i = 0; i < kJoinRunItems; ++i) mine += c[i];
  gf2_block_scan<long long, kJoinWaves>(mine, wave_sum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// d = a ^ p over the nw words of a row, the last one masked; lane `sub` of LANES takes the pairs of words sub, sub + LANES, ...
// -> the ones of this lane's words of d in the columns [wc0, wc1).  vec_a / vec_b / vec_d: see gf2_load2; an odd last word goes alone
template <int LANES>
__device__ __forceinline__ int join_xor_row(u64 *d, const u64 *a, const u64 *p, long long nw, u64 mlast, int vec_a, int vec_b, int vec_d,
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

// A run recomputes its partners and the sums of their counts before every position, then deals its OUTPUTS to groups of LANES lanes:
// output j of the run belongs to the position q found by bisection in the sums, and pairs position s = s0 + q of A with position
// p = l(s) + (j - pre[q]) of B.  The lanes of a wave so write consecutive rows of D whatever the sizes of the classes are.
template <int LANES>
__global__ void __launch_bounds__(kJoinThreads) gf2_join_scatter_kernel(const u64 *A, long long lda, const u64 *B, long long ldb, int ncols,
                                                                        const int *order_a, const int *ska, long long na,
                                                                        const int *order_b, const int *skb, long long nb,
                                                                        const long long *offsets, u64 *D, long long ldd, long long cap,
                                                                        int *ia, int *ib, int *wt, int wc0, int wc1, int vec_a, int vec_b,
                                                                        int vec_d) {
  __shared__ long long pre[kJoinRunRows];
  __shared__ int lpos[kJoinRunRows];
  __shared__ int stage[kJoinSpanKeys];
  __shared__ int span[2];
  __shared__ long long wave_sum[kJoinWaves];
  const long long off = offsets[blockIdx.x];
  if (off >= cap) return;  // the whole run lies behind the capacity: nothing of it is read
  const long long s0 = (long long)blockIdx.x * kJoinRunRows;
  int l[kJoinRunItems], c[kJoinRunItems];
  join_run_partners(ska, na, skb, nb, s0, stage, span, l, c);
  long long mine = 0, total;
#pragma unroll
  for (int i = 0; i < kJoinRunItems; ++i) mine += c[i];
  long long before = gf2_block_scan<long long, kJoinWaves>(mine, wave_sum, &total);
#pragma unroll
  for (int i = 0; i < kJoinRunItems; ++i) {
    const int q = kJoinRunItems * threadIdx.x + i;
    pre[q] = before;
    lpos[q] = l[i];
    before += c[i];
  }
  __syncthreads();
  const long long jmax = total < cap - off ? total : cap - off;  // outputs at or behind the capacity are skipped before a row is read
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const int sub = threadIdx.x % LANES;
  for (long long j = threadIdx.x / LANES; j < jmax; j += kJoinThreads / LANES) {  // the lanes of a group share j: they leave together
    const int q = gf2_find_position(pre, kJoinRunRows, j);
    const long long p = lpos[q] + (j - pre[q]);
    const int a = order_a[s0 + q], r = order_b[p];
    const long long at = off + j;
    int w = join_xor_row<LANES>(D + at * ldd, A + (long long)a * lda, B + (long long)r * ldb, nw, mlast, vec_a, vec_b, vec_d, sub, wc0, wc1);
#pragma unroll
    for (int d = LANES >> 1; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);  // over the lane group
    if (sub == 0) {
      if (ia) ia[at] = a;
      if (ib) ib[at] = r;
      if (wt) wt[at] = w;
    }
  }
}

#include "gf2_join_select.inc"  // gf2_join_weigh_kernel / gf2_join_select_scatter_kernel and their launchers: the weight-filtered join

}  // namespace

extern "C" hipError_t gf2k_join_count(const int *skeys_a, int nrows_a, const int *skeys_b, int nrows_b, long long *sums, long long *count,
                                      hipStream_t stream) {
  const JoinPlan plan = join_plan(nrows_a, nrows_b, 0, 0);
  if (plan.passes < 0 || nrows_a <= 0 || nrows_b <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_join_count_kernel, dim3((unsigned)plan.runs), dim3(kJoinThreads), 0, stream, skeys_a, (long long)nrows_a, skeys_b,
                     (long long)nrows_b, sums);
  hipLaunchKernelGGL(gf2_join_scan_kernel, dim3(1), dim3(kJoinThreads), 0, stream, sums, plan.runs, count);
  return hipGetLastError();
}

#define JOIN_SCATTER(LANES)                                                                                                            \
  hipLaunchKernelGGL((gf2_join_scatter_kernel<LANES>), grid, block, 0, stream, A, lda, B, ldb, ncols, order_a, skeys_a, (long long)nrows_a, \
                     order_b, skeys_b, (long long)nrows_b, offsets, D, ldd, (long long)cap, ia, ib, wt, wc0, wc1, vec_a, vec_b, vec_d)

extern "C" hipError_t gf2k_join_scatter(const u64 *A, long long lda, int nrows_a, const u64 *B, long long ldb, int nrows_b, int ncols,
                                        const int *order_a, const int *skeys_a, const int *order_b, const int *skeys_b,
                                        const long long *offsets, u64 *D, long long ldd, int cap, int *ia, int *ib, int *wt, int wc0, int wc1,
                                        int lanes, hipStream_t stream) {
  const JoinPlan plan = join_plan(nrows_a, nrows_b, ncols, 0);
  if (plan.passes < 0 || nrows_a <= 0 || nrows_b <= 0 || cap <= 0) return hipErrorInvalidValue;
  if (lanes < 0) lanes = plan.lanes;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_a = gf2_rows_aligned16(A, lda, nrows_a, nw), vec_b = gf2_rows_aligned16(B, ldb, nrows_b, nw),
            vec_d = gf2_rows_aligned16(D, ldd, cap, nw);
  const dim3 grid((unsigned)plan.runs), block(kJoinThreads);
  if (lanes == 1)
    JOIN_SCATTER(1);
  else if (lanes == 2)
    JOIN_SCATTER(2);
  else if (lanes == 8)
    JOIN_SCATTER(8);
  else if (lanes == 64)
    JOIN_SCATTER(64);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
