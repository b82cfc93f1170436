// gf2_sums.hip -- all XORs of p rows of a matrix in rank order, with their indices and weights, and the subsets of given ranks, on the
// device (include/m4ri_hip_sums.h; host side and contract: sums_host.cpp; order and plan: sums_plan.h).
//
//     D[t] = base ^ S[c_1] ^ ... ^ S[c_p], idx, wt for the subset of rank rank0 + t      gf2_subset_sums_kernel<1 | 2 | 8 | 64 lanes per row, S in LDS | S global>
//     idx[t * p ..] = the subset of rank rank0 + ranks[t]                                   gf2_unrank_subsets_kernel
//
// A workgroup takes `ranks` consecutive ranks (sums_plan).  Group g of its kSumsThreads / LANES lane groups unranks its first rank
// once and then walks on by a stride of one workgroup's groups with the carry chain of the order (sums_advance), so the lanes of a wave
// write consecutive rows.  Between two carries only c_1 moves: the XOR of base and the rows c_2 .. c_p stays in registers (up to
// kSumsCachedUnits 16-byte pieces per lane; the 64-lane kernels, whose rows have no bound, redo it per output), and an output is one
// read of a piece of S[c_1], one XOR, a popcount where weights are wanted, and one store.
//
// S in LDS: the workgroup first copies the n rows, and base as row n (zeros where there is none), into LDS, compact and with the excess
// bits of the last word cleared.  S global: the rows are read where they lie, with 16-byte accesses where every row starts on a
// 16-byte boundary; consecutive ranks read consecutive rows, and S stays in L2.
//
// Everything is integer arithmetic with one writer per output word and no atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_sums.h"
#include "sums_plan.h"

namespace {

// ---- rows

// two words of a row from word k on
struct SumsPair {
  u64 a, b;
};

// the words k and k + 1 of a row (0 for k + 1 where the row ends with k: an odd last word goes alone); vec: the rows of this operand
// start on 16-byte boundaries, so a pair is one 16-byte access
__device__ __forceinline__ SumsPair sums_load2(const u64 *row, long long k, long long nw, int vec) {
  SumsPair x;
  if (vec && k + 1 < nw) {
    const uint4 v = *reinterpret_cast<const uint4 *>(row + k);
    x.a = gf2_lo_hi(v.x, v.y);
    x.b = gf2_lo_hi(v.z, v.w);
  } else {
    x.a = row[k];
    x.b = 0;
    if (k + 1 < nw) x.b = row[k + 1];
  }
  return x;
}

// where the rows are: S (or its copy in LDS) and base (null: none)
struct SumsRows {
  const u64 *rows;
  long long ld;
  int vec;
  const u64 *base;
  int vec_base;
};

// the words k, k + 1 of base ^ S[c_first + 1] ^ ... ^ S[c_p] (first: 0 all p rows, 1 all but c_1)
__device__ __forceinline__ SumsPair sums_prefix(const SumsRows &r, unsigned c1, unsigned c2, unsigned c3, unsigned c4, int first, int p,
                                                long long k, long long nw) {
  SumsPair x = {0, 0};
  if (r.base) x = sums_load2(r.base, k, nw, r.vec_base);
  const unsigned c[kSumsMaxP] = {c1, c2, c3, c4};
#pragma unroll
  for (int i = 0; i < kSumsMaxP; ++i)
    if (i >= first && i < p) {
      const SumsPair y = sums_load2(r.rows + (long long)c[i] * r.ld, k, nw, r.vec);
      x.a ^= y.a;
      x.b ^= y.b;
    }
  return x;
}

// the pair of words from k on of an output row: masked, weighed, stored (d null: rows not stored) -> its ones in [wc0, wc1)
__device__ __forceinline__ int sums_emit(u64 *d, long long k, long long nw, u64 mlast, int vec_d, SumsPair x, int wc0, int wc1) {
  if (k + 1 < nw) {
    if (k + 1 == nw - 1) x.b &= mlast;
    if (d) {
      if (vec_d) {
        *reinterpret_cast<uint4 *>(d + k) = make_uint4((u32)x.a, (u32)(x.a >> 32), (u32)x.b, (u32)(x.b >> 32));
      } else {
        d[k] = x.a;
        d[k + 1] = x.b;
      }
    }
    return gf2_word_weight(x.a, k, wc0, wc1) + gf2_word_weight(x.b, k + 1, wc0, wc1);
  }
  x.a &= mlast;
  if (d) d[k] = x.a;
  return gf2_word_weight(x.a, k, wc0, wc1);
}

template <int LANES, bool STAGED>
__global__ void __launch_bounds__(kSumsThreads) gf2_subset_sums_kernel(const u64 *S, long long lds_, int n, const u64 *base, int ncols, int p,
                                                                       long long rank0, long long count, long long ranks, u64 *D,
                                                                       long long ldd, int *idx, int *wt, int wc0, int wc1, int vec_s,
                                                                       int vec_b, int vec_d) {
  extern __shared__ __attribute__((aligned(16))) u64 stage[];  // STAGED: n + 1 rows of nw words
  constexpr int UNITS = LANES == 64 ? 0 : LANES == 8 ? kSumsCachedUnits : 1;  // pieces of a row per lane (64 lanes: no bound)
  static_assert(2 * 8 * kSumsCachedUnits >= kLf2MidWords && 2 * 2 >= kLf2NarrowWords && 2 >= kLf2PieceWords, "a lane's pieces cover its row");
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  SumsRows r = {S, lds_, vec_s, base, vec_b};
  if (STAGED) {
    const int words = n * (int)nw;  // at most kSumsLdsBytes / 8
    for (int i = threadIdx.x; i < words; i += kSumsThreads) {
      const int row = i / (int)nw, k = i - row * (int)nw;
      const u64 x = S[(long long)row * lds_ + k];
      stage[i] = k == nw - 1 ? x & mlast : x;
    }
    for (int k = threadIdx.x; k < nw; k += kSumsThreads) stage[words + k] = base ? (k == nw - 1 ? base[k] & mlast : base[k]) : 0;
    __syncthreads();
    r = {stage, nw, 0, stage + words, 0};
  }
  constexpr int GROUPS = kSumsThreads / LANES;
  const int sub = threadIdx.x % LANES;
  const long long first = (long long)blockIdx.x * ranks;
  const long long end = first + ranks < count ? first + ranks : count;
  long long t = first + threadIdx.x / LANES;  // the lanes of a group share t: they leave together
  if (t >= end) return;
  const bool bits = D != nullptr || wt != nullptr;
  unsigned c[4];
  sums_unrank((unsigned long long)(rank0 + t), p, (unsigned)n, c);
  SumsPair pre[UNITS ? UNITS : 1];
  bool redo = true;
  for (; t < end; t += GROUPS) {
    int w = 0;
    if (bits) {
      u64 *d = D ? D + t * ldd : nullptr;
      if (UNITS) {
        const u64 *s1 = r.rows + (long long)c[0] * r.ld;
#pragma unroll
        for (int j = 0; j < (UNITS ? UNITS : 1); ++j) {
          const long long k = 2 * ((long long)sub + (long long)j * LANES);
          if (k < nw) {
            if (redo) pre[j] = sums_prefix(r, c[0], c[1], c[2], c[3], 1, p, k, nw);
            SumsPair x = sums_load2(s1, k, nw, r.vec);
            x.a ^= pre[j].a;
            x.b ^= pre[j].b;
            w += sums_emit(d, k, nw, mlast, vec_d, x, wc0, wc1);
          }
        }
      } else {
        for (long long k = 2ll * sub; k < nw; k += 2 * LANES)
          w += sums_emit(d, k, nw, mlast, vec_d, sums_prefix(r, c[0], c[1], c[2], c[3], 0, p, k, nw), wc0, wc1);
      }
#pragma unroll
      for (int o = LANES >> 1; o >= 1; o >>= 1) w += __shfl_xor(w, o, 64);  // over the lane group
    }
    if (sub == 0) {
      if (idx) {
#pragma unroll
        for (int i = 0; i < kSumsMaxP; ++i)
          if (i < p) idx[t * p + i] = (int)c[i];
      }
      if (wt) wt[t] = w;
    }
    redo = sums_advance(c, GROUPS);
  }
}

// one thread per rank
__global__ void __launch_bounds__(kSumsThreads) gf2_unrank_subsets_kernel(const int *ranks, int count, long long rank0, int p, int n,
                                                                          long long total, int *idx, int *bad) {
  const long long t = (long long)blockIdx.x * kSumsThreads + threadIdx.x;
  if (t >= count) return;
  const long long rel = ranks[t], rank = rank0 + rel;
  unsigned c[4] = {kSumsNone, kSumsNone, kSumsNone, kSumsNone};  // as ints: -1
  if (rel != -1) {
    if (rank >= 0 && rank < total)
      sums_unrank((unsigned long long)rank, p, (unsigned)n, c);
    else if (bad)
      *bad = 1;
  }
#pragma unroll
  for (int i = 0; i < kSumsMaxP; ++i)
    if (i < p) idx[t * p + i] = (int)c[i];
}

}  // namespace

#define SUMS_LAUNCH(LANES, STAGED)                                                                                                        \
  hipLaunchKernelGGL((gf2_subset_sums_kernel<LANES, STAGED>), grid, block, (STAGED) ? (size_t)plan.lds : 0, stream, S, lds_, n, base, ncols, \
                     p, rank0, count, plan.ranks, D, ldd, idx, wt, wc0, wc1, vec_s, vec_b, vec_d)

extern "C" hipError_t gf2k_subset_sums(const u64 *S, long long lds_, int n, const u64 *base, int ncols, int p, long long rank0,
                                       long long count, u64 *D, long long ldd, int *idx, int *wt, int wc0, int wc1, int global_s,
                                       hipStream_t stream) {
  const SumsPlan plan = sums_plan(n, ncols, p, count);
  if (plan.id < 0 || count <= 0 || n < p || (!D && !idx && !wt)) return hipErrorInvalidValue;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_s = gf2_rows_aligned16(S, lds_, n, nw), vec_b = base ? gf2_rows_aligned16(base, nw, 1, nw) : 0,
            vec_d = D ? gf2_rows_aligned16(D, ldd, count, nw) : 0;
  const dim3 grid((unsigned)plan.groups), block(kSumsThreads);
  const int id = global_s ? (plan.id | 4) : plan.id;
  switch (id) {
    case 0: SUMS_LAUNCH(1, true); break;
    case 1: SUMS_LAUNCH(2, true); break;
    case 2: SUMS_LAUNCH(8, true); break;
    case 3: SUMS_LAUNCH(64, true); break;
    case 4: SUMS_LAUNCH(1, false); break;
    case 5: SUMS_LAUNCH(2, false); break;
    case 6: SUMS_LAUNCH(8, false); break;
    default: SUMS_LAUNCH(64, false); break;
  }
  return hipGetLastError();
}

extern "C" hipError_t gf2k_unrank_subsets(const int *ranks, int count, long long rank0, int p, int n, int *idx, int *bad, hipStream_t stream) {
  const long long total = sums_count(n, p);
  if (count <= 0 || total < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_unrank_subsets_kernel, dim3((unsigned)((count + kSumsThreads - 1) / kSumsThreads)), dim3(kSumsThreads), 0, stream,
                     ranks, count, rank0, p, n, total, idx, bad);
  return hipGetLastError();
}
