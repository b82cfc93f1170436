// philox.h -- the generator of the device draws (include/m4ri_hip_draw.h; kernels: gf2_draw.hip) and the
// per-word rules built on it, in ONE place: the kernels call these functions and nothing else to make a value, and tests/draw_emu.cpp
// compiles this very file for the CPU under the host compiler's sanitizers.  Plain C++: no inline assembly, no builtin that a host
// compiler lacks, so the same text gives the same bits on both sides.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): a counter of four 32-bit
// words, a key of two, ten rounds.  The key is (seed low 32, seed high 32).  Counter word 3 is a TAG that separates the entries, so
// that no two of them ever see the same block of a seed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GF2_DRAW_FN __host__ __device__ __forceinline__
#else
#define GF2_DRAW_FN inline
#endif

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // the multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // the key increments
constexpr int kPhiloxRounds = 10;

constexpr uint32_t kDrawTagBernoulli = 1, kDrawTagIndices = 2, kDrawTagSubsets = 3, kDrawTagPermutation = 4;
constexpr int kDrawPermKeyBits = 30;  // the key of the permutation: what the class sort takes

struct Philox4 {
  uint32_t x0, x1, x2, x3;
};

GF2_DRAW_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < kPhiloxRounds; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;  // 32 x 32 -> 64
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return {c0, c1, c2, c3};
}

// the block of a 64-bit position under a seed
GF2_DRAW_FN Philox4 draw_block(uint64_t seed, uint64_t at, uint32_t c2, uint32_t tag) {
  return philox4x32_10((uint32_t)at, (uint32_t)(at >> 32), c2, tag, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// mulhi64(X, n) for X = lo | hi << 32 and n < 2^32: the high 64 bits of the 128-bit product, a value in [0, n).  Exact and
// branch-free; the bias of a value is below n / 2^64.  (hi * n + a carry below 2^32 stays below 2^64)
GF2_DRAW_FN uint32_t draw_below(uint32_t lo, uint32_t hi, uint32_t n) {
  const uint64_t t = (uint64_t)lo * n;
  const uint64_t u = (uint64_t)hi * n + (t >> 32);
  return (uint32_t)(u >> 32);
}

// ---- Bernoulli: word widx of the noise, bit i set with probability thr / 2^32
// Call q of the word gives the bit-planes R[2q] = x0 | x1 << 32 and R[2q + 1] = x2 | x3 << 32; bit i of plane m is bit m of the
// 32-bit number U_i, and bit i of the word is U_i < thr.  The comparison runs bit-sliced, least significant plane first:
//     lt = thr_m ? (~R[m] | lt) : (~R[m] & lt)
// Planes below the lowest set bit of thr leave lt == 0, so the calls that give only such planes are not made.
GF2_DRAW_FN int draw_bernoulli_first_call(uint32_t thr) { return thr ? __builtin_ctz(thr) >> 1 : 16; }

// The functions below hold the COMPLEMENT nlt = ~lt, so that no plane has to be inverted: with nt = zero or all ones for thr_m = 1
// or 0, the rule reads nlt = thr_m ? (R[m] & nlt) : (R[m] | nlt), which is the majority of (R[m], nlt, nt): branch-free, one
// three-input bit operation per plane and half word.
GF2_DRAW_FN uint64_t draw_bernoulli_plane(uint64_t nlt, uint64_t plane, uint32_t thr_bit) {
  const uint64_t nt = (uint64_t)thr_bit - 1;
  return (plane & nlt) | (nt & (plane | nlt));
}

GF2_DRAW_FN uint64_t draw_bernoulli_word(uint64_t seed, uint64_t widx, uint32_t thr) {
  uint64_t nlt = ~(uint64_t)0;
  for (int q = draw_bernoulli_first_call(thr); q < 16; ++q) {
    const Philox4 x = draw_block(seed, widx, (uint32_t)q, kDrawTagBernoulli);
    nlt = draw_bernoulli_plane(nlt, (uint64_t)x.x0 | ((uint64_t)x.x1 << 32), (thr >> (2 * q)) & 1);
    nlt = draw_bernoulli_plane(nlt, (uint64_t)x.x2 | ((uint64_t)x.x3 << 32), (thr >> (2 * q + 1)) & 1);
  }
  return ~nlt;
}

// ---- indices: draws t = 2p and t = 2p + 1 share the block of p
GF2_DRAW_FN void draw_index_pair(uint64_t seed, uint64_t p, uint32_t n, uint32_t *even, uint32_t *odd) {
  const Philox4 x = draw_block(seed, p, 0, kDrawTagIndices);
  *even = draw_below(x.x0, x.x1, n);
  *odd = draw_below(x.x2, x.x3, n);
}

// ---- subsets: what position `at` = g * k + t draws in round a
GF2_DRAW_FN uint32_t draw_subset_candidate(uint64_t seed, uint64_t at, uint32_t round, uint32_t n) {
  const Philox4 x = draw_block(seed, at, round, kDrawTagSubsets);
  return draw_below(x.x0, x.x1, n);
}

// ---- permutation: the sort key of i
GF2_DRAW_FN uint32_t draw_perm_key(uint64_t seed, uint32_t i) {
  return draw_block(seed, i, 0, kDrawTagPermutation).x0 & ((1u << kDrawPermKeyBits) - 1);
}
