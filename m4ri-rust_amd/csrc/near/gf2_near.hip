// gf2_near.hip -- the Hamming-distance search between two pools on the device (include/m4ri_hip_near.h; host side and contract:
// near_host.cpp; plan: near_plan.h).  All NA * NB pairs are weighed with both operands on chip:
//
//     the hits of every cell (row of A, chunk of B), one int64 per cell                       gf2_near_kernel<W, kNearCount> / gf2_near_wide_kernel
//     hit counts -> hit offsets in the order (ia, ib), *hits                                  gf2_near_scan_kernel
//     D[offset + rank] = A[ia] ^ B[ib], ia, ib, wt for the hits below the capacity            gf2_near_kernel<W, kNearSelect> / gf2_near_wide_kernel
//     the minimum of the keys (d << 32 | j) of every cell; the minimum over a row's chunks     gf2_near_kernel<W, kNearNearest> / ..., gf2_near_fold_kernel
//
// The register kernels (W = 1, 2, 4, 8, 16 words of range): a workgroup owns kNearBlockRows rows of A and one chunk of B.  A lane keeps
// the range's words of two rows of A in registers, masked to the range.  The chunk goes through LDS in tiles of 16 KiB, masked as
// well, and every lane of a wave reads the same tile row at the same address (a broadcast, 16 bytes per read): per pair and 32 bits of
// range one XOR and one popcount that adds to the running weight, and nothing else but the test of the window or the minimum.  The wide
// kernels (a range of more than 16 words) keep nothing on chip: a lane walks its row of A and the rows of the chunk in global memory.
//
// The flags exclude pairs by their row numbers.  A tile of B is classed once per workgroup: no pair excluded (the loop above), some
// (the same loop with the test of every pair), all (the tile is skipped, before it is read).
//
// Everything is integer arithmetic with one writer per output word and no atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "../../../include/m4ri_hip_near.h"
#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "gf2_near.h"
#include "near_plan.h"

namespace {

enum { kNearCount = 0, kNearSelect = 1, kNearNearest = 2 };
constexpr int kNearWaves = kNearThreads / 64;
constexpr int kNearScanItems = 8;  // cells per lane and round of the scan
constexpr u32 kNearNoKey = ~0u;
constexpr u64 kNearNoKey64 = ~0ull;

// what the kernels are given: the operands, the window as its lower end and its length, the chunks, the cells, the outputs
struct NearArgs {
  const u64 *A;
  long long lda, na;
  const u64 *B;
  long long ldb, nb;
  int ncols, wc0, wc1, flags, wlo;
  u32 span;
  long long chunks, chunk_rows;
  long long *cells;
  u64 *D;
  long long ldd, cap;
  int *ia, *ib, *wt;
};

// ---- word-level helpers: plain values and pointers, no thread index (tests/test_near_helpers_cpu.py runs their text on the CPU)

// is a pair of weight w a hit of the window [wlo, wlo + span]?  One unsigned comparison: a w below wlo wraps to a large number
__device__ __forceinline__ int near_in_window(int w, int wlo, u32 span) { return (u32)(w - wlo) <= span; }

// do the flags exclude the pair of row i of A and row j of B?
__device__ __forceinline__ int near_excluded(long long i, long long j, int flags) {
  return (flags & GF2_NEAR_UPPER) ? j <= i : (flags & GF2_NEAR_OFF_DIAGONAL) ? j == i : 0;
}

// what the rows [t0, t1) of B are to the rows [r0, r1) of A under the flags: 0 no pair is excluded, 1 some may be, 2 all are
__device__ __forceinline__ int near_tile_class(long long r0, long long r1, long long t0, long long t1, int flags) {
  if (flags & GF2_NEAR_UPPER) return t1 - 1 <= r0 ? 2 : t0 > r1 - 1 ? 0 : 1;
  if (flags & GF2_NEAR_OFF_DIAGONAL) return t0 < r1 && r0 < t1 ? 1 : 0;
  return 0;
}

// the key of a pair inside its chunk: the weight (at most 1024) above the row's place in the chunk (below 2^21).  The minimum of the
// keys of a lane is its nearest row, the lowest one among equals.  kNearNoKey is above every key
__device__ __forceinline__ u32 near_pack_key(int w, u32 jrel) { return ((u32)w << kNearKeyShift) + jrel; }
// the key of a pair among all rows of B, j0 the first row of the chunk: (d << 32 | j), kNearNoKey64 for kNearNoKey
__device__ __forceinline__ u64 near_chunk_key(u32 key, long long j0) {
  if (key == kNearNoKey) return kNearNoKey64;
  return ((u64)(key >> kNearKeyShift) << 32) | (u64)(j0 + (long long)(key & ((1u << kNearKeyShift) - 1)));
}
__device__ __forceinline__ u64 near_wide_key(int w, long long j) { return ((u64)(u32)w << 32) | (u64)j; }
__device__ __forceinline__ int near_key_dist(u64 key) { return key == kNearNoKey64 ? -1 : (int)(key >> 32); }
__device__ __forceinline__ int near_key_index(u64 key) { return key == kNearNoKey64 ? -1 : (int)(key & 0xFFFFFFFFull); }

// the ones of a ^ b over the W words of a range that both have been masked to
template <int W>
__device__ __forceinline__ int near_weight(const u64 (&a)[W], const u64 (&b)[W]) {
  int w = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) w += __popcll(a[k] ^ b[k]);
  return w;
}

// the ones of x ^ y in the columns [wc0, wc1), read from the rows themselves: only the words [first, end) of the range are read
__device__ __forceinline__ int near_row_weight(const u64 *x, const u64 *y, long long first, long long end, int wc0, int wc1) {
  int w = 0;
  for (long long k = first; k < end; ++k) w += __popcll((x[k] ^ y[k]) & gf2_word_mask(k, wc0, wc1));
  return w;
}

// hit `at` of the call: the whole row A[i] ^ B[j] with the excess bits of its last word zero (D null: not stored), and its entries
__device__ __forceinline__ void near_emit(const NearArgs &p, long long at, long long i, long long j, int w) {
  if (p.D) {
    const long long nw = ((long long)p.ncols + 63) >> 6;
    const u64 mlast = ~0ull >> (63 - (int)(((long long)p.ncols - 1) & 63));
    const u64 *x = p.A + i * p.lda, *y = p.B + j * p.ldb;
    u64 *d = p.D + at * p.ldd;
    for (long long k = 0; k < nw; ++k) d[k] = (x[k] ^ y[k]) & (k == nw - 1 ? mlast : ~0ull);
  }
  if (p.ia) p.ia[at] = (int)i;
  if (p.ib) p.ib[at] = (int)j;
  if (p.wt) p.wt[at] = w;
}

// ---- what a lane keeps for one of its rows of A, and what it does with a pair

struct NearRow {
  long long i;    // the row of A
  long long off;  // select: the first place of the cell's hits
  int lim;        // select: the hits of the cell that are written
  int cnt;        // count, select: the hits so far
  u32 best;       // nearest: the lowest key so far
};

// the hits of the cell of row s.i and chunk c that lie below the capacity, from the scanned counts (cells[last + 1] is the total)
__device__ __forceinline__ void near_cell_window(const NearArgs &p, long long c, NearRow &s) {
  s.off = 0;
  s.lim = 0;
  if (s.i >= p.na) return;
  const long long cell = near_cell(s.i, p.chunks, c);
  const long long off = p.cells[cell], own = p.cells[cell + 1] - off;
  if (own == 0 || off >= p.cap) return;
  s.off = off;
  s.lim = (int)(own < p.cap - off ? own : p.cap - off);  // a cell has at most kNearMaxChunkRows pairs
}

template <int MODE>
__device__ __forceinline__ void near_take(const NearArgs &p, NearRow &s, long long j, u32 jrel, int w, bool admitted) {
  if (MODE == kNearCount) {
    s.cnt += admitted && near_in_window(w, p.wlo, p.span);
  } else if (MODE == kNearSelect) {
    if (admitted && near_in_window(w, p.wlo, p.span)) {
      if (s.cnt < s.lim) near_emit(p, s.off + s.cnt, s.i, j, w);
      ++s.cnt;
    }
  } else {
    const u32 key = near_pack_key(w, jrel);
    const u32 lower = key < s.best ? key : s.best;
    s.best = admitted ? lower : s.best;
  }
}

// what the cell keeps of its lane's work
template <int MODE>
__device__ __forceinline__ void near_leave(const NearArgs &p, long long c, long long j0, const NearRow &s) {
  if (s.i >= p.na) return;
  if (MODE == kNearCount) p.cells[near_cell(s.i, p.chunks, c)] = s.cnt;
  if (MODE == kNearNearest) p.cells[near_cell(s.i, p.chunks, c)] = (long long)near_chunk_key(s.best, j0);
}

// ---- the register kernels

// row jj of the tile, 16 bytes per read where a row has a pair of words
template <int W>
__device__ __forceinline__ void near_tile_row(const u64 *tile, int jj, u64 (&b)[W]) {
  if (W == 1) {
    b[0] = tile[jj];
  } else {
    const ulonglong2 *t = reinterpret_cast<const ulonglong2 *>(tile) + (long long)jj * (W / 2);
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
      const ulonglong2 v = t[k];
      b[2 * k] = v.x;
      b[2 * k + 1] = v.y;
    }
  }
}

// the n rows of the tile, which are the rows t0 .. of B, against the lane's rows of A
template <int W, int MODE, bool FLAGGED>
__device__ __forceinline__ void near_walk(const NearArgs &p, const u64 *tile, int n, long long t0, long long j0,
                                          const u64 (&a)[kNearLaneRows][W], NearRow (&s)[kNearLaneRows]) {
  constexpr int kRowsInFlight = W >= 8 ? 2 : 4;  // tile rows whose LDS reads are issued ahead of their use
#pragma unroll kRowsInFlight
  for (int jj = 0; jj < n; ++jj) {
    u64 b[W];
    near_tile_row<W>(tile, jj, b);
    const long long j = t0 + jj;
#pragma unroll
    for (int r = 0; r < kNearLaneRows; ++r) {
      const int w = near_weight<W>(a[r], b);
      near_take<MODE>(p, s[r], j, (u32)(j - j0), w, FLAGGED ? !near_excluded(s[r].i, j, p.flags) : true);
    }
  }
}

template <int W, int MODE>
__global__ void __launch_bounds__(kNearThreads) gf2_near_kernel(NearArgs p) {
  constexpr int kTileRows = kNearTileBytes / (8 * W);
  __shared__ __attribute__((aligned(16))) u64 tile[kNearTileBytes / 8];
  const long long r0 = (long long)blockIdx.x * kNearBlockRows, c = blockIdx.y;
  const long long j0 = near_chunk_begin(c, p.chunk_rows), j1 = near_chunk_end(c, p.chunk_rows, p.nb);
  const long long first = near_first_word(p.wc0, p.wc1);
  const int words = (int)(near_end_word(p.wc0, p.wc1) - first);  // at most W; the words from `words` on are zero and are not read
  NearRow s[kNearLaneRows];
  u64 a[kNearLaneRows][W];
  int writes = 0;
#pragma unroll
  for (int r = 0; r < kNearLaneRows; ++r) {
    s[r].i = r0 + (long long)r * kNearThreads + threadIdx.x;
    s[r].cnt = 0;
    s[r].best = kNearNoKey;
#pragma unroll
    for (int k = 0; k < W; ++k)
      a[r][k] = s[r].i < p.na && k < words ? p.A[s[r].i * p.lda + first + k] & gf2_word_mask(first + k, p.wc0, p.wc1) : 0;
    if (MODE == kNearSelect) {
      near_cell_window(p, c, s[r]);
      writes |= s[r].lim > 0;
    }
  }
  if (MODE == kNearSelect && !__syncthreads_or(writes)) return;  // no hit of this workgroup below the capacity: B is not read
  for (long long t0 = j0; t0 < j1; t0 += kTileRows) {
    const int n = (int)(j1 - t0 < kTileRows ? j1 - t0 : kTileRows);
    const int cls = near_tile_class(r0, r0 + kNearBlockRows, t0, t0 + n, p.flags);  // the same in every lane
    if (cls == 2) continue;
    __syncthreads();  // the tile before this one has been read by every lane
    for (int e = threadIdx.x; e < n * W; e += kNearThreads) {
      const int k = e % W;
      tile[e] = k < words ? p.B[(t0 + e / W) * p.ldb + first + k] & gf2_word_mask(first + k, p.wc0, p.wc1) : 0;
    }
    __syncthreads();
    if (cls == 0)
      near_walk<W, MODE, false>(p, tile, n, t0, j0, a, s);
    else
      near_walk<W, MODE, true>(p, tile, n, t0, j0, a, s);
  }
#pragma unroll
  for (int r = 0; r < kNearLaneRows; ++r) near_leave<MODE>(p, c, j0, s[r]);
}

// ---- the wide kernels: a lane owns one row of A and walks the chunk in global memory; no LDS, no barrier

template <int MODE>
__global__ void __launch_bounds__(kNearThreads) gf2_near_wide_kernel(NearArgs p) {
  const long long c = blockIdx.y;
  const long long j0 = near_chunk_begin(c, p.chunk_rows), j1 = near_chunk_end(c, p.chunk_rows, p.nb);
  const long long first = near_first_word(p.wc0, p.wc1), end = near_end_word(p.wc0, p.wc1);
  NearRow s;
  s.i = (long long)blockIdx.x * kNearWideBlockRows + threadIdx.x;
  s.cnt = 0;
  if (s.i >= p.na) return;
  if (MODE == kNearSelect) {
    near_cell_window(p, c, s);
    if (s.lim == 0) return;
  }
  u64 best = kNearNoKey64;  // the weight of a wide range does not fit the packed key
  const u64 *x = p.A + s.i * p.lda;
  for (long long j = j0; j < j1; ++j) {
    if (near_excluded(s.i, j, p.flags)) continue;
    const int w = near_row_weight(x, p.B + j * p.ldb, first, end, p.wc0, p.wc1);
    if (MODE == kNearNearest) {
      const u64 key = near_wide_key(w, j);
      if (key < best) best = key;
    } else {
      near_take<MODE>(p, s, j, 0, w, true);
    }
  }
  if (MODE == kNearCount) p.cells[near_cell(s.i, p.chunks, c)] = s.cnt;
  if (MODE == kNearNearest) p.cells[near_cell(s.i, p.chunks, c)] = (long long)best;
}

// ---- the scan of the cells and the fold of the chunk minima

// one workgroup: v[k] becomes the sum of the values before k for k < n, v[n] and *total the sum of all
__global__ void __launch_bounds__(kNearThreads) gf2_near_scan_kernel(long long *v, long long n, long long *total) {
  __shared__ long long wave_sum[kNearWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long long running = 0;
  for (long long b0 = 0; b0 < n; b0 += kNearThreads * kNearScanItems) {
    const long long k0 = b0 + (long long)kNearScanItems * threadIdx.x;
    long long x[kNearScanItems], mine = 0;
#pragma unroll
    for (int i = 0; i < kNearScanItems; ++i) {
      x[i] = k0 + i < n ? v[k0 + i] : 0;
      mine += x[i];
    }
    // the wave scan written out, not gf2_block_scan: with the call this kernel compiles to other code (40 -> 48 VGPRs)
    long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    long long before = running + incl - mine, all = 0;
#pragma unroll
    for (int wv = 0; wv < kNearWaves; ++wv) {
      if (wv < wave) before += wave_sum[wv];
      all += wave_sum[wv];
    }
#pragma unroll
    for (int i = 0; i < kNearScanItems; ++i) {
      if (k0 + i < n) v[k0 + i] = before;
      before += x[i];
    }
    running += all;
    __syncthreads();  // before the next round writes wave_sum
  }
  if (threadIdx.x == 0) {
    v[n] = running;
    *total = running;
  }
}

// idx[i], dist[i] <- the minimum of the keys of the chunks of row i
__global__ void __launch_bounds__(kNearThreads) gf2_near_fold_kernel(const long long *cells, long long na, long long chunks, int *idx,
                                                                     int *dist) {
  const long long i = (long long)blockIdx.x * kNearThreads + threadIdx.x;
  if (i >= na) return;
  u64 best = kNearNoKey64;
  for (long long c = 0; c < chunks; ++c) {
    const u64 key = (u64)cells[near_cell(i, chunks, c)];
    if (key < best) best = key;
  }
  if (idx) idx[i] = near_key_index(best);
  if (dist) dist[i] = near_key_dist(best);
}

NearArgs near_args(const NearOperands *o, const NearPlan &plan, int wlo, int whi, long long *cells) {
  NearArgs p = {};
  p.A = o->A, p.lda = o->lda, p.na = o->nrows_a;
  p.B = o->B, p.ldb = o->ldb, p.nb = o->nrows_b;
  p.ncols = o->ncols, p.wc0 = o->wc0, p.wc1 = o->wc1, p.flags = o->flags;
  p.wlo = wlo, p.span = (u32)whi - (u32)wlo;
  p.chunks = plan.chunks, p.chunk_rows = plan.chunk_rows;
  p.cells = cells;
  return p;
}

#define NEAR_LAUNCH(W, MODE) hipLaunchKernelGGL((gf2_near_kernel<W, MODE>), grid, block, 0, stream, p)

template <int MODE>
hipError_t near_launch(const NearPlan &plan, const NearArgs &p, hipStream_t stream) {
  const dim3 grid((unsigned)plan.row_blocks, (unsigned)plan.chunks), block(kNearThreads);
  switch (plan.kernel) {
    case 1: NEAR_LAUNCH(1, MODE); break;
    case 2: NEAR_LAUNCH(2, MODE); break;
    case 4: NEAR_LAUNCH(4, MODE); break;
    case 8: NEAR_LAUNCH(8, MODE); break;
    case 16: NEAR_LAUNCH(16, MODE); break;
    case 0: hipLaunchKernelGGL((gf2_near_wide_kernel<MODE>), grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t gf2k_near_count(const NearOperands *o, int wlo, int whi, long long *cells, long long *hits, hipStream_t stream) {
  const NearPlan plan = near_plan(o->nrows_a, o->nrows_b, o->ncols, o->wc0, o->wc1);
  if (plan.kernel < 0 || o->nrows_a <= 0 || o->nrows_b <= 0) return hipErrorInvalidValue;
  const hipError_t e = near_launch<kNearCount>(plan, near_args(o, plan, wlo, whi, cells), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gf2_near_scan_kernel, dim3(1), dim3(kNearThreads), 0, stream, cells, (long long)o->nrows_a * plan.chunks, hits);
  return hipGetLastError();
}

extern "C" hipError_t gf2k_near_select(const NearOperands *o, int wlo, int whi, const long long *cells, uint64_t *D, long long ldd, int cap,
                                       int *ia, int *ib, int *wt, hipStream_t stream) {
  const NearPlan plan = near_plan(o->nrows_a, o->nrows_b, o->ncols, o->wc0, o->wc1);
  if (plan.kernel < 0 || o->nrows_a <= 0 || o->nrows_b <= 0 || cap <= 0) return hipErrorInvalidValue;
  NearArgs p = near_args(o, plan, wlo, whi, const_cast<long long *>(cells));  // the select kernels only read them
  p.D = D, p.ldd = ldd, p.cap = cap, p.ia = ia, p.ib = ib, p.wt = wt;
  return near_launch<kNearSelect>(plan, p, stream);
}

extern "C" hipError_t gf2k_nearest(const NearOperands *o, long long *cells, int *idx, int *dist, hipStream_t stream) {
  const NearPlan plan = near_plan(o->nrows_a, o->nrows_b, o->ncols, o->wc0, o->wc1);
  if (plan.kernel < 0 || o->nrows_a <= 0 || o->nrows_b <= 0) return hipErrorInvalidValue;
  const hipError_t e = near_launch<kNearNearest>(plan, near_args(o, plan, 0, 0, cells), stream);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)(((long long)o->nrows_a + kNearThreads - 1) / kNearThreads);
  hipLaunchKernelGGL(gf2_near_fold_kernel, dim3(blocks), dim3(kNearThreads), 0, stream, cells, (long long)o->nrows_a, plan.chunks, idx, dist);
  return hipGetLastError();
}
