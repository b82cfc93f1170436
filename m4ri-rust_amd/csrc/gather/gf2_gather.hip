// gf2_gather.hip -- rows and columns of a device matrix selected by a DEVICE index array (include/m4ri_hip_gather.h; host side and
// contract: gather_host.cpp; plan: gather_plan.h).
//
//   rows:     D[i]    (^)= S[idx[i]]        i < D.nrows      gf2_gather_rows_kernel, a word-level kernel
//   columns:  D[r][j]   =  S[r][idx[j]]     j < D.ncols      gf2_gather_cols_kernel, one workgroup per band of 64 rows
//
// An index of -1 is "no source" (zeros; with accumulate: unchanged); any other value outside the source is treated the same way, never
// dereferenced, and reported by a plain store of 1 to *bad.
//
// THE COLUMN KERNEL keeps the band in LDS COLUMN-MAJOR: T[c] is one 64-bit word, bit r of it is S[r0 + r][c].  A bit gather then is a
// word gather: lane j reads T[idx[64 w + j]] -- one random 8-byte LDS read per 64 output bits -- and a 64 x 64 bit transposition (the
// butterfly of gf2_transpose_kernel) turns the 64 words of the wave into word w of the band's 64 output rows.
//   phase 1  the 1024 threads load the band 16 word columns at a time, the 16 lanes of a row on 128 consecutive bytes, and put word k
//            of row r at T[64 k + (r + k) mod 64]: the raw words of a 64 x 64 block already lie in the 64 words that will hold its
//            columns.  All loads of the band are independent and one barrier ends them.  Then each of the 16 waves takes whole blocks,
//            lane = row, transposes them in registers and stores T[64 k + lane] in place; a second barrier, and T is complete.
//   phase 2  step s covers the word columns 16 s .. 16 s + 15 of D, one per wave: gather, transpose, lane = row, into staging buffer
//            s mod 2; a barrier; the 1024 threads store the 64 rows x 16 words, 128 consecutive bytes per row.  Two buffers make one
//            barrier per step enough: the barrier of step s + 1 lies between the reads of buffer s mod 2 and its next writes.  The
//            indices of the next step are loaded before the current one is worked on.
// LDS banks: the rotation (r + k) mod 64 spreads the 16 lanes of a row, which write 512 bytes apart, over 16 different pairs of
// banks, and the 64 lanes that read a block down its rows over 64 consecutive words.  The staging buffers hold word k of row r at
// 16 r + (k + r) mod 16 for the same reason, both ways.  The reads of T go where the indices say; equal indices broadcast.
// Every word of S and D is accessed by 8-byte loads and stores, so rows need only be 8-byte aligned.  Words of S are read only for
// rows below nrows and word columns below ceil(s_ncols / 64); bits of S's last word beyond s_ncols land in entries of T that no index
// can name.  D is written in whole words of its ceil(d_ncols / 64) per row: lanes beyond d_ncols contribute zeros.
#include <hip/hip_runtime.h>

#include <mutex>
#include <set>
#include <utility>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gather_plan.h"
#include "gf2_gather.h"

namespace {

// blockDim = (pieces, rows), 256 threads; rows walk grid.x, the pieces of a row grid.y, both with a stride loop.  A piece is a 16-byte
// pair of words when vec (every row of D and S starts on a 16-byte boundary: the launcher decides), else one word; the last word of a
// row is always handled alone under its mask, so no access reaches past the row's ceil(ncols / 64) words.
__global__ void __launch_bounds__(256) gf2_gather_rows_kernel(u64 *D, long long ldd, const u64 *S, long long lds_, long long d_nrows,
                                                              int s_nrows, int ncols, const int *idx, int accumulate, int vec, int *bad) {
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const long long units = vec ? (nw + 1) >> 1 : nw;
  for (long long r = (long long)blockIdx.x * blockDim.y + threadIdx.y; r < d_nrows; r += (long long)gridDim.x * blockDim.y) {
    for (long long u = (long long)blockIdx.y * blockDim.x + threadIdx.x; u < units; u += (long long)gridDim.y * blockDim.x) {
      const int src = idx[r];
      const bool ok = (unsigned)src < (unsigned)s_nrows;
      if (!ok && src != -1 && bad && u == 0) *bad = 1;
      if (!ok && accumulate) continue;
      u64 *d = D + r * ldd;
      const u64 *s = ok ? S + (long long)src * lds_ : nullptr;
      const long long k = vec ? 2 * u : u;
      if (vec && k + 1 < nw) {
        u64 v0 = 0, v1 = 0;
        if (ok) {
          const uint4 x = *reinterpret_cast<const uint4 *>(s + k);
          v0 = gf2_lo_hi(x.x, x.y);
          v1 = gf2_lo_hi(x.z, x.w);
        }
        if (k + 1 == nw - 1) v1 &= mlast;
        uint4 *p = reinterpret_cast<uint4 *>(d + k);
        if (accumulate) {
          const uint4 o = *p;
          v0 ^= gf2_lo_hi(o.x, o.y);
          v1 ^= gf2_lo_hi(o.z, o.w);
        }
        *p = make_uint4((u32)v0, (u32)(v0 >> 32), (u32)v1, (u32)(v1 >> 32));
      } else {
        u64 v = ok ? s[k] : 0ull;
        if (k == nw - 1) v &= mlast;
        d[k] = accumulate ? (d[k] ^ v) : v;
      }
    }
  }
}

// 64 x 64 bits across a wave, N blocks side by side (their exchange rounds overlap): lane r holds row r of each block on entry and
// column r on return (six rounds, as gf2_transpose_kernel)
template <int N>
__device__ __forceinline__ void gather_transpose64(u64 (&x)[N], int lane) {
#pragma unroll
  for (int b = 5; b >= 0; --b) {
    const int d = 1 << b;
    const u64 mask = ~0ull / ((1ull << d) + 1);  // d low bits of every 2 d: 0x00000000FFFFFFFF ... 0x5555555555555555
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const u64 y = __shfl_xor(x[i], d, 64);
      x[i] = (lane & d) ? ((x[i] & ~mask) | ((y >> d) & mask)) : ((x[i] & mask) | ((y << d) & ~mask));
    }
  }
}

// One workgroup of 16 waves per band of 64 rows (the last band may end early).  Dynamic LDS: T[64 sw], then two staging buffers of
// 64 x 16 words.
__global__ void __launch_bounds__(kGatherThreads) gf2_gather_cols_kernel(u64 *D, long long ldd, int d_ncols, const u64 *S, long long lds_,
                                                                         int s_ncols, long long nrows, const int *idx, int *bad) {
  extern __shared__ __attribute__((aligned(16))) u64 gather_lds[];
  constexpr int CW = kGatherStageWords, WAVES = kGatherThreads / 64;
  static_assert(CW == 16 && WAVES == CW && kGatherThreads == kGatherBandRows * CW, "a thread per staged word, a wave per staged word column");
  const int sw = (s_ncols + 63) >> 6, dw = (d_ncols + 63) >> 6;
  u64 *T = gather_lds;
  u64 *stage = gather_lds + (long long)64 * sw;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int srow = tid >> 4, sk = tid & 15;  // this thread's row and word when the 1024 threads cover 64 rows x 16 words
  const long long r0 = (long long)blockIdx.x * kGatherBandRows;
  const int live = (int)(nrows - r0 < kGatherBandRows ? nrows - r0 : kGatherBandRows);

  // ---- phase 1: the band into T
  const u64 *srcrow = S + (r0 + (srow < live ? srow : 0)) * lds_;
  for (int k0 = 0; k0 < sw; k0 += 4 * CW) {
    u64 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + CW * q + sk;
      v[q] = (k < sw && srow < live) ? srcrow[k] : 0ull;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + CW * q + sk;
      if (k < sw) T[64 * k + ((srow + k) & 63)] = v[q];
    }
  }
  __syncthreads();
  for (int k = wave; k < sw; k += 2 * WAVES) {  // uniform over the wave; two blocks at a time
    const int k2 = k + WAVES < sw ? k + WAVES : k;
    u64 x[2] = {T[64 * k + ((lane + k) & 63)], T[64 * k2 + ((lane + k2) & 63)]};
    gather_transpose64(x, lane);
    T[64 * k + lane] = x[0];
    if (k2 != k) T[64 * k2 + lane] = x[1];
  }
  __syncthreads();

  // ---- phase 2: gather, transpose back, store
  const int steps = (dw + CW - 1) / CW;
  long long j = 64ll * wave + lane;  // the output column of this lane in the current step
  int c = j < d_ncols ? idx[j] : -1;
  for (int s = 0; s < steps; ++s) {
    const bool active = CW * s + wave < dw;  // uniform over the wave
    const int cur = c;
    j += 64 * CW;
    c = (s + 1 < steps && j < d_ncols) ? idx[j] : -1;
    u64 *buf = stage + (s & 1) * (kGatherBandRows * CW);
    if (active) {
      const bool ok = (unsigned)cur < (unsigned)s_ncols;
      if (!ok && cur != -1 && bad && blockIdx.x == 0) *bad = 1;
      u64 x[1] = {ok ? T[cur] : 0ull};
      gather_transpose64(x, lane);
      buf[CW * lane + ((wave + lane) & (CW - 1))] = x[0];
    }
    __syncthreads();
    const int w = CW * s + sk;
    if (w < dw && srow < live) D[(r0 + srow) * ldd + w] = buf[CW * srow + ((sk + srow) & (CW - 1))];
  }
}

// the dynamic-LDS limit of a kernel is per device and costs host time: once per device
hipError_t gather_lds_limit_once(const void *kernel, int bytes) {
  static std::mutex mu;
  static std::set<int> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (done.count(dev)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.insert(dev);
  return e;
}

}  // namespace

extern "C" hipError_t gf2k_gather_rows(u64 *D, long long ldd, const u64 *S, long long lds_, int d_nrows, int s_nrows, int ncols,
                                       const int *idx, int accumulate, int *bad, hipStream_t stream) {
  if (d_nrows <= 0 || ncols <= 0) return hipSuccess;
  const long long nw = ((long long)ncols + 63) >> 6;
  // 16-byte pieces only where every row of both matrices starts on a 16-byte boundary (an empty S is never read)
  const int vec = (s_nrows <= 0 || gf2_rows_aligned16(S, lds_, s_nrows, nw)) && gf2_rows_aligned16(D, ldd, d_nrows, nw);
  const long long units = vec ? (nw + 1) >> 1 : nw;
  int wx = 1;  // pieces across a workgroup: the power of two that covers a row, 256 at the most
  while (wx < units && wx < 256) wx <<= 1;
  const int ry = 256 / wx;
  const long long gx = ((long long)d_nrows + ry - 1) / ry, gy = units / wx;  // gy rounds down: the stride loop takes the rest
  const dim3 grid((unsigned)(gx > (1 << 22) ? (1 << 22) : gx), (unsigned)(gy < 1 ? 1 : gy > 65535 ? 65535 : gy));
  hipLaunchKernelGGL(gf2_gather_rows_kernel, grid, dim3(wx, ry), 0, stream, D, ldd, S, lds_, (long long)d_nrows, s_nrows, ncols, idx,
                     accumulate ? 1 : 0, vec, bad);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_gather_cols(u64 *D, long long ldd, int d_ncols, const u64 *S, long long lds_, int s_ncols, int nrows,
                                       const int *idx, int *bad, hipStream_t stream) {
  if (nrows <= 0 || d_ncols <= 0) return hipSuccess;
  const GatherColsPlan plan = gather_cols_plan(nrows, s_ncols, d_ncols);
  if (plan.path != 0) return hipErrorInvalidValue;
  const hipError_t e = gather_lds_limit_once(reinterpret_cast<const void *>(&gf2_gather_cols_kernel), (int)kGatherLdsBudget);
  if (e != hipSuccess) return e;
  const long long bands = ((long long)nrows + plan.rows - 1) / plan.rows;  // < 2^25
  hipLaunchKernelGGL(gf2_gather_cols_kernel, dim3((unsigned)bands), dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, stream, D, ldd,
                     d_ncols, S, lds_, s_ncols, (long long)nrows, idx, bad);
  return hipGetLastError();
}
