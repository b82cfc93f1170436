// gf2_merge4.inc -- the merge of a plan step with a virtual level: all four Strassen levels folded into C in one launch.
// Included by gf2_kernels.hip behind gf2_strassen_merge3_kernel (static_for, kStrassenFoldTo).
//
// gf2_strassen_merge3_kernel (7 groups) followed by gf2_strassen_merge_kernel writes the seven level-1 products and reads them
// back: 2 x 7/4 of C on top of the one read of the 2401 leaf products and the one write of C that the result needs.  One thread
// cannot keep the 256 results of its word position (512 registers), so here they live in LDS:
//   * a workgroup of 7 waves takes a block of 64 consecutive word positions (idx = r * w + c, lane = position: every load and
//     store is a 512-byte run) and walks the blocks grid-stride;
//   * wave v takes top-level group q0 = v: the per-thread walk of gf2_strassen_merge3_kernel over that group's 343 leaves
//     (q1 a run-time loop, masked folds, non-temporal loads) ends with the group's 64 results in registers;
//   * it adds them into the sums of the one or two quadrants of C the group feeds (kStrassenFoldTo[q0]) with LDS atomics whose
//     result is unused -- two waves may hit one word at once.  Layout [quadrant][k][lane]: 64 lanes, 64 consecutive words;
//   * after a barrier all waves write the 256 x 64 words to C (non-temporal) and clear the sums as they read them, so that the
//     barrier behind the write-out is also the one in front of the next block's adds.
// Every leaf word is read once, every word of C written once, and no workgroup waits for another.
// The sums take 4 x 64 x 64 x 8 B = 128 KiB of dynamic LDS: one workgroup per CU.
// Lanes past the last position skip their loads, adds and stores but take part in every barrier; the block loop's bounds are
// the same for the whole workgroup.

constexpr int kMerge4Waves = 7;
constexpr int kMerge4Threads = kMerge4Waves * 64;
constexpr int kMerge4LdsBytes = 4 * 64 * 64 * 8;

__global__ __launch_bounds__(kMerge4Threads) void gf2_strassen_merge4_kernel(u64 *__restrict__ dst, long long ldd, long long dstStride,
                                                                             const u64 *__restrict__ src, long long lds_,
                                                                             long long srcStride, int h, int w, int accumulate) {
  // h, w: rows / words of one INPUT product (a sixteenth of the destination in each dimension); blockIdx.y: batch element
  extern __shared__ u64 merge4_sums[];  // [4 quadrants of C][64 sub-blocks k][64 positions]
  const int lane = threadIdx.x & 63, q0 = threadIdx.x >> 6;
  const u64 *M = src + ((long long)blockIdx.y * 7 + q0) * 343 * srcStride;
  u64 *Cq = dst + (long long)blockIdx.y * dstStride;
  const long long total = (long long)h * w, nblocks = (total + 63) >> 6;
  for (int i = threadIdx.x; i < 4 * 64 * 64; i += kMerge4Threads) merge4_sums[i] = 0;
  __syncthreads();
  for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const long long idx = blk * 64 + lane;
    const bool live = idx < total;
    const int r = (int)(idx / w), c = (int)(idx % w);
    if (live) {
      const u64 *Mp = M + (long long)r * lds_ + c;
      u64 z[64];
      static_for<64>([&](auto K) { z[decltype(K)::value] = 0; });
      // (the body of gf2_strassen_merge3_kernel<true>, which see)
#pragma unroll 1
      for (int q1 = 0; q1 < 7; ++q1) {
        u64 y[16];
        static_for<16>([&](auto J) { y[decltype(J)::value] = 0; });
        const u64 *Mq = Mp + (long long)(49 * q1) * srcStride;
        static_for<7>([&](auto Q2) {
          constexpr int q2 = decltype(Q2)::value;
          u64 m[7];
          static_for<7>([&](auto Q3) {
            constexpr int q3 = decltype(Q3)::value;
            m[q3] = __builtin_nontemporal_load(&Mq[(long long)(7 * q2 + q3) * srcStride]);
          });
          const u64 f[4] = {m[0] ^ m[3] ^ m[4] ^ m[6], m[2] ^ m[4], m[1] ^ m[3], m[0] ^ m[1] ^ m[2] ^ m[5]};
          constexpr int t0 = kStrassenFoldTo[q2][0], t1 = kStrassenFoldTo[q2][1];
          static_for<4>([&](auto J) {
            constexpr int j = decltype(J)::value;
            y[t0 * 4 + j] ^= f[j];
            if (t1 >= 0) y[(t1 < 0 ? 0 : t1) * 4 + j] ^= f[j];
          });
        });
        const int u0 = kStrassenFoldTo[q1][0], u1 = kStrassenFoldTo[q1][1];
        static_for<4>([&](auto U) {
          constexpr int u = decltype(U)::value;
          const u64 mask = (u == u0 || u == u1) ? ~0ull : 0ull;
          static_for<16>([&](auto J) {
            constexpr int j = decltype(J)::value;
            z[u * 16 + j] ^= y[j] & mask;
          });
        });
      }
      // the group's 64 results into the one or two quadrants of C it feeds (the same for the whole wave)
      const int v0 = kStrassenFoldTo[q0][0], v1 = kStrassenFoldTo[q0][1];
      unsigned long long *s0 = reinterpret_cast<unsigned long long *>(merge4_sums) + v0 * 4096 + lane;
      static_for<64>([&](auto K) { atomicXor(s0 + decltype(K)::value * 64, z[decltype(K)::value]); });
      if (v1 >= 0) {
        unsigned long long *s1 = reinterpret_cast<unsigned long long *>(merge4_sums) + v1 * 4096 + lane;
        static_for<64>([&](auto K) { atomicXor(s1 + decltype(K)::value * 64, z[decltype(K)::value]); });
      }
    }
    __syncthreads();
    // write-out: result j = 64 * quadrant + k in chunks of eight per wave, the loads of a chunk ahead of its stores.  The address
    // is merge3's with one more level: sub-block (R, Cc) of 16 x 16, h rows x w words each.
    for (int j0 = q0 * 8; j0 < 256; j0 += kMerge4Waves * 8) {
      u64 v[8];
      u64 *pd[8];
      static_for<8>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int j = j0 + i, qd = j >> 6;
        const int R = 8 * (qd >> 1) + 4 * ((j >> 5) & 1) + 2 * ((j >> 3) & 1) + ((j >> 1) & 1);
        const int Cc = 8 * (qd & 1) + 4 * ((j >> 4) & 1) + 2 * ((j >> 2) & 1) + (j & 1);
        pd[i] = Cq + (long long)(r + R * h) * ldd + (long long)Cc * w + c;
        v[i] = merge4_sums[j * 64 + lane];
        merge4_sums[j * 64 + lane] = 0;
        if (accumulate && live) v[i] ^= *pd[i];
      });
      if (live) static_for<8>([&](auto I) { __builtin_nontemporal_store(v[decltype(I)::value], pd[decltype(I)::value]); });
    }
    __syncthreads();
  }
}
