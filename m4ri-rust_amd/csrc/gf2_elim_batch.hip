// gf2_elim_batch.hip -- elimination of a whole stack of small matrices in one launch (include/m4ri_hip.h:
// gf2_echelonize_batch_dev, gf2_inverse_batch_dev; argument checks and the plan: elim_batch_host.cpp).
//
// A batch is `batch` matrices of m rows stored one below the other; matrix b is rows [b * m, (b + 1) * m).  Each matrix gets the
// contract of gf2_echelonize_dev / gf2_inverse_dev; nothing here talks to the host, so the call is one asynchronous launch.
//
//   m <= 64        wave kernel: one wave per matrix, lane r holds row r in W registers (W = 1, 2, 4, 8 or 16 words), no LDS, no
//                  barrier.  Per column: ballot over the lanes >= rank whose bit is set, the first of them is the pivot, its words
//                  are broadcast with v_readlane, lane `rank` and the pivot lane exchange rows, every other lane with the bit adds
//                  the pivot row.  Four waves = four matrices per workgroup; they never meet.
//   64 < m <= 512  LDS kernel: one workgroup per matrix, one thread per row (a multiple of 64 threads), the matrix in LDS with an
//                  odd row stride.  Two barriers per pivot column, one per column without a pivot (see the kernel).
//
// The inverse runs the same kernels on [A | I]: the identity is made in registers / LDS, never read from memory, and the right half
// goes to Ainv only when the rank is n.
//
// WHICH WORDS ARE TOUCHED.  Of every row only the aw = ceil(ncols / 64) words of the matrix are loaded and stored (the 16-byte forms
// are taken only when both of their words are among them and the row is 16-byte aligned); rows are addressed as (b * m + r) * ld in 64 bits.  Lanes >= m, waves
// beyond the batch and threads >= m neither load nor store.
#include <hip/hip_runtime.h>

#include <atomic>

#include "api_internal.h"
#include "gf2_kernels.h"

typedef uint64_t u64;
typedef uint32_t u32;

namespace {

constexpr int kWaveThreads = GF2K_ELIM_BATCH_WAVE_THREADS;  // four waves = four matrices per workgroup
constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ u64 rdlane64(u64 v, int lane) {  // lane must be wave-uniform
  const int l = __builtin_amdgcn_readfirstlane(lane);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 lo_hi(u32 lo, u32 hi) { return (u64)lo | ((u64)hi << 32); }

// S: the stack that is read, D: the stack that is written (echelon form: the same; inverse: Ainv).  aw: words of a row in memory;
// INV: W = 2, word 1 is the identity.  limit <= 64 * aw columns are eliminated, the words behind them follow.
template <int W, bool INV>
__global__ __launch_bounds__(kWaveThreads) void gf2_elim_batch_wave_kernel(const u64 *S, long long lds_, u64 *D, long long ldd, int m,
                                                                           int aw, int limit, int full, long long batch, int *ranks,
                                                                           int *pivcols, int P, int *singular) {
  static_assert(!INV || W == 2, "the inverse of a matrix of at most 64 rows is one word of A and one of the identity");
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * (kWaveThreads / 64) + (threadIdx.x >> 6);
  if (b >= batch) return;  // whole waves leave: nothing below synchronises
  u64 row[W];
#pragma unroll
  for (int k = 0; k < W; ++k) row[k] = 0;
  if (lane < m) {
    const u64 *src = S + (b * m + lane) * lds_;
    const bool wide = !(reinterpret_cast<uintptr_t>(src) & 15);  // gf2_dmat_alloc gives one-word rows ld = 1; views may sit anywhere
    if constexpr (W == 1 || INV) {
      row[0] = src[0];
      if (INV) row[W - 1] = 1ull << lane;
    } else {
#pragma unroll
      for (int k = 0; k < W; k += 2) {
        if (k + 1 < aw && wide) {
          const uint4 x = *reinterpret_cast<const uint4 *>(src + k);
          row[k] = lo_hi(x.x, x.y);
          row[k + 1] = lo_hi(x.z, x.w);
        } else {
          if (k < aw) row[k] = src[k];
          if (k + 1 < aw) row[k + 1] = src[k + 1];
        }
      }
    }
  }
  int rank = 0, mypiv = -1;  // lane i ends up holding pivot row i and remembers its column
#pragma unroll
  for (int w = 0; w < W; ++w) {  // unrolled: row[] is indexed by constants only and stays in registers
    const int cend = limit - w * 64 < 64 ? limit - w * 64 : 64;
    for (int j = 0; j < cend && rank < m; ++j) {
      const u64 bit = 1ull << j;
      const u64 cand = __ballot((row[w] & bit) != 0 && lane >= rank);
      if (!cand) continue;
      const int p = __builtin_ctzll(cand);
      u64 pv[W];  // the pivot row; its words left of w are zero, like those of every row >= rank
#pragma unroll
      for (int k = w; k < W; ++k) pv[k] = rdlane64(row[k], p);
      if (p != rank) {
#pragma unroll
        for (int k = w; k < W; ++k) {
          const u64 rv = rdlane64(row[k], rank);
          if (lane == p) row[k] = rv;
          if (lane == rank) row[k] = pv[k];
        }
      }
      // after the exchange lane p holds what was row `rank`: every lane looks at its bit again
      if (lane != rank && (row[w] & bit) != 0 && (full || lane > rank)) {
#pragma unroll
        for (int k = w; k < W; ++k) row[k] ^= pv[k];
      }
      if (lane == rank) mypiv = w * 64 + j;
      ++rank;
    }
  }
  if (INV) {
    const int sing = rank < m;
    if (singular && lane == 0) singular[b] = sing;
    if (!sing && lane < m) D[(b * m + lane) * ldd] = row[W - 1];
    return;
  }
  if (lane < m) {
    u64 *dst = D + (b * m + lane) * ldd;
    const bool wide = !(reinterpret_cast<uintptr_t>(dst) & 15);
    if constexpr (W == 1) {
      dst[0] = row[0];
    } else {
#pragma unroll
      for (int k = 0; k < W; k += 2) {
        if (k + 1 < aw && wide) {
          *reinterpret_cast<uint4 *>(dst + k) = make_uint4((u32)row[k], (u32)(row[k] >> 32), (u32)row[k + 1], (u32)(row[k + 1] >> 32));
        } else {
          if (k < aw) dst[k] = row[k];
          if (k + 1 < aw) dst[k + 1] = row[k + 1];
        }
      }
    }
  }
  if (ranks && lane == 0) ranks[b] = rank;
  if (pivcols && lane < P) pivcols[b * P + lane] = lane < rank ? mypiv : -1;
}

// One workgroup per matrix, thread r owns row r.  LDS: the rows (hw = aw words, or 2 * aw with the identity, at the odd stride hw | 1:
// the threads' reads of one word column fall on distinct banks), the pivot row of the current column, the waves' first candidates
// (two sets, used in turn) and the pivot columns -- gf2_elim_batch_plan (elim_batch_host.cpp) computes the same sum as out[2].
//
// A column costs two barriers.  (A) behind the waves' ballots; then everybody knows the pivot row p.  The wave that owns row p moves it,
// one word per lane: into `pivrow`, into row `rank`, and row `rank`'s words into row p.  (B) behind that; then every thread whose bit is
// set adds `pivrow` to its own row.  No third barrier: a thread reads only its own row for the next ballot, rows p and `rank` are written
// between (A) and (B) when nobody reads a row, and `pivrow` is rewritten only behind the next (A).  A column without a pivot leaves
// before (B); the candidates of the next column go to the other set, which nobody reads any more (its readers have passed (A) since).
// rank, p and the trip count are the same in every thread, whatever the matrix holds: every barrier is reached by the whole workgroup.
template <bool INV>
__global__ __launch_bounds__(512) void gf2_elim_batch_lds_kernel(const u64 *S, long long lds_, u64 *D, long long ldd, int m, int aw,
                                                                 int limit, int full, int *ranks, int *pivcols, int P, int *singular) {
  extern __shared__ __attribute__((aligned(16))) u64 M[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
  const int hw = INV ? 2 * aw : aw, stride = hw | 1;
  u64 *pivrow = M + m * stride;
  int *s_first = reinterpret_cast<int *>(pivrow + stride);  // [2][8]
  int *s_piv = s_first + 16;                                // [m]
  const long long b = blockIdx.x;
  const u64 *src = S + b * m * lds_;
  for (int idx = tid; idx < m * aw; idx += nthreads) {
    const int r = idx / aw, k = idx - r * aw;
    M[r * stride + k] = src[(long long)r * lds_ + k];
    if (INV) M[r * stride + aw + k] = k == (r >> 6) ? 1ull << (r & 63) : 0ull;
  }
  __syncthreads();
  u64 *mine = M + tid * stride;  // dereferenced by threads < m only
  int rank = 0;
  for (int c = 0; c < limit && rank < m; ++c) {
    const int cw = c >> 6;
    const u64 bit = 1ull << (c & 63);
    const u64 cand = __ballot(tid < m && tid >= rank && (mine[cw] & bit) != 0);
    int *sf = s_first + (c & 1) * 8;
    if (lane == 0) sf[wave] = cand ? wave * 64 + __builtin_ctzll(cand) : kNone;
    __syncthreads();  // (A)
    int p = kNone;
    for (int w = 0; w < nwaves; ++w) p = min(p, sf[w]);
    if (p == kNone) continue;  // no pivot in this column: the same decision in every thread
    if (wave == (p >> 6)) {
      for (int k = cw + lane; k < hw; k += 64) {  // both rows are zero left of word cw
        const u64 a = M[p * stride + k], o = M[rank * stride + k];
        pivrow[k] = a;
        M[p * stride + k] = o;
        M[rank * stride + k] = a;
      }
    }
    if (tid == 0) s_piv[rank] = c;
    __syncthreads();  // (B)
    if (tid < m && tid != rank && (full || tid > rank) && (mine[cw] & bit) != 0)
      for (int k = cw; k < hw; ++k) mine[k] ^= pivrow[k];
    ++rank;
  }
  __syncthreads();
  if (INV) {
    if (singular && tid == 0) singular[b] = rank < m;
    if (rank < m) return;
  }
  u64 *dst = D + b * m * ldd;
  for (int idx = tid; idx < m * aw; idx += nthreads) {
    const int r = idx / aw, k = idx - r * aw;
    dst[(long long)r * ldd + k] = M[r * stride + (INV ? aw : 0) + k];
  }
  if (INV) return;
  if (ranks && tid == 0) ranks[b] = rank;
  if (pivcols)
    for (int i = tid; i < P; i += nthreads) pivcols[b * P + i] = i < rank ? s_piv[i] : -1;
}

// LDS above the 64 KiB a kernel gets without asking (512 rows of 17 words): once per device and kernel
template <class K>
hipError_t allow_lds(K kernel, int which, int bytes) {
  constexpr int kMaxDev = 1024, kMost = 160 * 1024;
  static std::atomic<unsigned char> done[2][kMaxDev];
  if (bytes <= 64 * 1024) return hipSuccess;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= kMaxDev) return hipErrorInvalidDevice;
  if (done[which][dev].load(std::memory_order_acquire)) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMost);
  if (e == hipSuccess) done[which][dev].store(1, std::memory_order_release);
  return e;
}

}  // namespace

// The variant is gf2_elim_batch_plan's choice alone (elim_batch_host.cpp); the caller has checked every argument.  inverse: S is the
// stack A, D the stack Ainv, ncols = m = n.
extern "C" hipError_t gf2k_elim_batch(const u64 *S, long long lds_, u64 *D, long long ldd, int m, int ncols, int limit, int full,
                                      int inverse, long long batch, int *ranks, int *pivcols, int *singular, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  long long plan[4];
  const int variant = gf2_elim_batch_plan(m, ncols, inverse, plan);
  if (variant < 0 || limit < 1 || limit > ncols) return hipErrorInvalidValue;
  const int aw = (ncols + 63) >> 6, P = m < limit ? m : limit, threads = (int)plan[0], lds = (int)plan[2];
  const long long grid = (batch + plan[1] - 1) / plan[1];
  if (grid > 0x7fffffffll) return hipErrorInvalidValue;
  const dim3 g((unsigned)grid), t((unsigned)threads);
#define GF2K_WAVE(W, INV)                                                                                                          \
  hipLaunchKernelGGL((gf2_elim_batch_wave_kernel<W, INV>), g, t, 0, s, S, lds_, D, ldd, m, aw, limit, full, batch, ranks, pivcols, \
                     P, singular)
  switch (variant) {
    case GF2K_ELIM_BATCH_WAVE1: GF2K_WAVE(1, false); break;
    case GF2K_ELIM_BATCH_WAVE2: GF2K_WAVE(2, false); break;
    case GF2K_ELIM_BATCH_WAVE4: GF2K_WAVE(4, false); break;
    case GF2K_ELIM_BATCH_WAVE8: GF2K_WAVE(8, false); break;
    case GF2K_ELIM_BATCH_WAVE16: GF2K_WAVE(16, false); break;
    case GF2K_ELIM_BATCH_WAVE_INV: GF2K_WAVE(2, true); break;
    case GF2K_ELIM_BATCH_LDS: {
      if (hipError_t e = allow_lds(&gf2_elim_batch_lds_kernel<false>, 0, lds)) return e;
      hipLaunchKernelGGL(gf2_elim_batch_lds_kernel<false>, g, t, lds, s, S, lds_, D, ldd, m, aw, limit, full, ranks, pivcols, P,
                         singular);
      break;
    }
    case GF2K_ELIM_BATCH_LDS_INV: {
      if (hipError_t e = allow_lds(&gf2_elim_batch_lds_kernel<true>, 1, lds)) return e;
      hipLaunchKernelGGL(gf2_elim_batch_lds_kernel<true>, g, t, lds, s, S, lds_, D, ldd, m, aw, limit, full, ranks, pivcols, P,
                         singular);
      break;
    }
    default: return hipErrorInvalidValue;
  }
#undef GF2K_WAVE
  return hipGetLastError();
}
