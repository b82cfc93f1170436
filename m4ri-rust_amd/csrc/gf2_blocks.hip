// gf2_blocks.hip -- rectangular bit-block copy between arbitrary bit offsets (include/m4ri_hip.h: gf2_copy_block_dev and the
// calls built on it; contract and host side: blocks_host.cpp).
//
//   D[dr + i][dc + j] (^)= S[sr + i][sc + j]      i < nrows, j < ncols
//
// The launcher moves both base pointers to the first word a row of the rectangle touches, so the kernel sees the bit offsets
// dcb = dc % 64 and scb = sc % 64 alone.  A row of the rectangle lives in ndw = ceil((dcb + ncols) / 64) destination words and
// nsw = ceil((scb + ncols) / 64) source words.  Destination word k takes its bits from the source words k + qoff and k + qoff + 1
// (qoff = 0 when scb >= dcb, else -1), funnelled by t = (scb - dcb) mod 64; t = 0 is a word copy.
//
// One thread owns one 16-byte-aligned PAIR of destination words (k0, k0 + 1): the pairing follows the ADDRESS of the row, not the
// word index, so a row that starts on an odd word (an odd dc / 64, or an odd ld on an odd row) begins with a lone word and the
// interior still goes out in 16-byte stores.  A pair that lies inside the rectangle with all 128 bits is stored whole; the first and
// the last word of a row are read-modify-written under their masks (one word is both when ndw = 1), so every destination word is
// written by exactly one thread and bits of D outside the rectangle keep their values.
//
// WHICH WORDS ARE TOUCHED.  A destination word is accessed only with an index k in [0, ndw) and a source word only with an index in
// [0, nsw): every load and store below sits behind exactly that test (h0 / h1 for the destination, in() for the source; the 16-byte
// forms are taken only when BOTH of their words pass it).  By the definition of ndw and nsw each of those words holds at least one
// bit of the rectangle, so it lies inside the caller's matrix; the word after the last one -- which may be past the end of the
// allocation when the rectangle ends with the buffer -- is never formed into an address that is dereferenced.
//
// S and D are not __restrict__: they may be views of one buffer whose rectangles share a WORD without sharing a bit (columns 0..99 ->
// 100..199).  The owner of that destination word rewrites the source bits in it unchanged, and 8-byte accesses do not tear, so a
// reader sees the same source bits before and after.
#include <hip/hip_runtime.h>

#include "gf2_kernels.h"

typedef uint64_t u64;
typedef uint32_t u32;

namespace {

__device__ __forceinline__ u64 lo_hi(u32 lo, u32 hi) { return (u64)lo | ((u64)hi << 32); }

// one destination word under its mask m (never 0); z: bits to clear besides (the excess bits of the matrix's last word)
__device__ __forceinline__ void put_word(u64 *p, u64 v, u64 m, u64 z, int accumulate) {
  if (m == ~0ull && !accumulate) {
    *p = v;
    return;
  }
  const u64 old = *p;
  *p = accumulate ? ((old ^ (v & m)) & ~z) : ((old & ~(m | z)) | (v & m));
}

// blockDim = (words, rows), 256 threads; rows walk grid.x, pairs of a row grid.y (both with a stride loop: neither a row count of
// 2^20 and more nor a very wide row overflows a launch dimension).
__global__ void __launch_bounds__(256) gf2_copy_block_kernel(u64 *D, long long ldd, int dcb, const u64 *S, long long lds_, int scb,
                                                             long long nrows, int ncols, int accumulate, int zero_tail) {
  const long long ndw = ((long long)dcb + ncols + 63) >> 6, nsw = ((long long)scb + ncols + 63) >> 6;
  const int t = (scb - dcb) & 63;
  const long long qoff = scb >= dcb ? 0 : -1;
  const u64 mfirst = ~0ull << dcb;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)dcb + ncols - 1) & 63));
  const u64 ztail = zero_tail ? ~mlast : 0ull;
  for (long long r = (long long)blockIdx.x * blockDim.y + threadIdx.y; r < nrows; r += (long long)gridDim.x * blockDim.y) {
    u64 *d = D + r * ldd;
    const u64 *s = S + r * lds_;
    const int odd = (int)((reinterpret_cast<uintptr_t>(d) >> 3) & 1);  // the row's first word is the upper half of its 16 bytes
    const long long units = (ndw + odd + 1) >> 1;
    for (long long u = (long long)blockIdx.y * blockDim.x + threadIdx.x; u < units; u += (long long)gridDim.y * blockDim.x) {
      const long long k0 = 2 * u - odd, k1 = k0 + 1;  // k0 <= ndw - 1 and k1 >= 0 by the bound on u
      const bool h0 = k0 >= 0, h1 = k1 < ndw;
      u64 m0 = h0 ? ~0ull : 0ull, m1 = h1 ? ~0ull : 0ull;
      if (k0 == 0) m0 &= mfirst;
      if (k1 == 0) m1 &= mfirst;
      if (k0 == ndw - 1) m0 &= mlast;
      if (k1 == ndw - 1) m1 &= mlast;
      u64 v0 = 0, v1 = 0;
      if (t == 0) {  // nsw == ndw, source word k feeds destination word k
        if (h0 && h1 && !(reinterpret_cast<uintptr_t>(s + k0) & 15)) {
          const uint4 x = *reinterpret_cast<const uint4 *>(s + k0);
          v0 = lo_hi(x.x, x.y);
          v1 = lo_hi(x.z, x.w);
        } else {
          if (h0) v0 = s[k0];
          if (h1) v1 = s[k1];
        }
      } else {
        const long long q = k0 + qoff;
        const u64 w0 = (h0 && q >= 0 && q < nsw) ? s[q] : 0ull;
        const u64 w1 = (q + 1 >= 0 && q + 1 < nsw) ? s[q + 1] : 0ull;
        const u64 w2 = (h1 && q + 2 < nsw) ? s[q + 2] : 0ull;
        v0 = (w0 >> t) | (w1 << (64 - t));
        v1 = (w1 >> t) | (w2 << (64 - t));
      }
      if ((m0 & m1) == ~0ull) {  // both words whole: d + k0 is 16-byte aligned by the choice of k0
        uint4 *p = reinterpret_cast<uint4 *>(d + k0);
        if (accumulate) {
          const uint4 o = *p;
          v0 ^= lo_hi(o.x, o.y);
          v1 ^= lo_hi(o.z, o.w);
        }
        *p = make_uint4((u32)v0, (u32)(v0 >> 32), (u32)v1, (u32)(v1 >> 32));
      } else {
        if (h0) put_word(d + k0, v0, m0, k0 == ndw - 1 ? ztail : 0ull, accumulate);
        if (h1) put_word(d + k1, v1, m1, k1 == ndw - 1 ? ztail : 0ull, accumulate);
      }
    }
  }
}

}  // namespace

extern "C" hipError_t gf2k_copy_block(u64 *D, long long ldd, long long dr, long long dc, const u64 *S, long long lds_, long long sr,
                                      long long sc, int nrows, int ncols, int accumulate, int zero_tail, hipStream_t stream) {
  if (nrows <= 0 || ncols <= 0) return hipSuccess;
  const int dcb = (int)(dc & 63), scb = (int)(sc & 63);
  u64 *d = D + dr * ldd + (dc >> 6);
  const u64 *s = S + sr * lds_ + (sc >> 6);
  const long long ndw = ((long long)dcb + ncols + 63) >> 6;
  const long long units = (ndw + 2) >> 1;  // the most a row can have (it starts on an odd word)
  int wx = 1;  // pairs across a workgroup: the power of two that covers a row, 256 at the most
  while (wx < units && wx < 256) wx <<= 1;
  const int ry = 256 / wx;
  const long long gx = ((long long)nrows + ry - 1) / ry, gy = units / wx;  // gy rounds down: the stride loop takes the odd pair
  const dim3 grid((unsigned)(gx > (1 << 22) ? (1 << 22) : gx), (unsigned)(gy < 1 ? 1 : gy > 65535 ? 65535 : gy));
  hipLaunchKernelGGL(gf2_copy_block_kernel, grid, dim3(wx, ry), 0, stream, d, ldd, dcb, s, lds_, scb, (long long)nrows, ncols,
                     accumulate ? 1 : 0, zero_tail ? 1 : 0);
  return hipGetLastError();
}
