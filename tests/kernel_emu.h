// kernel_emu.h -- stand-ins for the HIP names that the word-level kernels use, so that their shipped text compiles with the host
// compiler and runs thread by thread under its address and undefined-behaviour sanitizers (blocks_emu.cpp, kernels_emu.cpp).
// A launch is a loop over the grid and the block, one thread after the other: there is no ordering between threads to observe, no
// wave and no LDS.  Only kernels that need none of these are run this way (tests/test_kernels_cpu.py holds the partition).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

typedef uint64_t u64;
typedef uint32_t u32;

struct alignas(16) uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
struct alignas(16) u32x4 { uint32_t x, y, z, w; };  // the clang vector type of the non-temporal 16-byte accesses
struct alignas(8) int2 { int x, y; };
static inline int2 make_int2(int a, int b) { return int2{a, b}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, gridDim, blockDim;

#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(...)
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
// the host compiler has no non-temporal builtins: plain accesses of the same width and alignment
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))

typedef int hipError_t;
typedef void *hipStream_t;
#define hipSuccess 0
#define hipErrorInvalidValue 1
#define hipGetLastError() 0

static long g_threads = 0;
static long g_block_threads = 256;  // what every launch must use (all these kernels are written for 256); 0: anything up to 1024
// k: a kernel's name, or a parenthesised template instance
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...)                                                        \
  do {                                                                                                              \
    gridDim = grid; blockDim = block;                                                                               \
    const long nthr_ = (long)blockDim.x * blockDim.y * blockDim.z;                                                  \
    if (nthr_ < 1 || nthr_ > 1024 || (g_block_threads && nthr_ != g_block_threads) || !gridDim.x || !gridDim.y || !gridDim.z || gridDim.y > 65535u ||        \
        gridDim.z > 65535u) { printf("bad launch shape\n"); abort(); }                                              \
    for (unsigned bz_ = 0; bz_ < gridDim.z; ++bz_) for (unsigned by_ = 0; by_ < gridDim.y; ++by_)                   \
      for (unsigned bx_ = 0; bx_ < gridDim.x; ++bx_)                                                                \
        for (unsigned tz_ = 0; tz_ < blockDim.z; ++tz_) for (unsigned ty_ = 0; ty_ < blockDim.y; ++ty_)             \
          for (unsigned tx_ = 0; tx_ < blockDim.x; ++tx_) {                                                         \
            blockIdx = dim3(bx_, by_, bz_); threadIdx = dim3(tx_, ty_, tz_); ++g_threads; k(__VA_ARGS__); }         \
  } while (0)
