// gf2_find.hip -- the lookup of every row of A among the rows of B through a hash table (include/m4ri_hip_find.h; host side and
// contract: find_host.cpp; plan, hash and slot arithmetic: find_plan.h).
//
//   fill:    every entry = kFindEmpty, every count = 0, *count = 0                   gf2_find_fill_kernel
//   build:   row j of B walks its probe sequence to the slot of its class, leaves     gf2_find_build_kernel<lane | wave per row>
//            the lowest row there and adds one to the slot's count
//   lookup:  row i of A walks the same sequence: idx[i] = the entry's row and         gf2_find_lookup_kernel<lane | wave per row>
//            mult[i] = the slot's count, or -1 and 0 at the first empty slot; *count
//
// The bits of a word of the range are read through gf2_word_mask (gf2_dev_words.h) alone.  Rows are read with 8-byte loads and 64-bit
// offsets: only the words that hold a column of the range, the first and the last of them masked, and a compare reads nothing behind
// the first word that differs.
//
// THE SLOT OF A CLASS.  Equal rows have one hash and walk one sequence of slots.  An occupied slot never empties and its occupant is
// only ever replaced by an equal row (a 64-bit minimum among entries of one tag), so what a row sees on its way -- slots of other
// classes -- every equal row sees too, in whatever order they arrive: all of them stop at the same slot, the first that was empty or
// theirs.  The minimum of their entries and the sum of their ones do not depend on the order either.  The layout of the table does
// (which class took which slot of a chain), idx, mult and *count do not: two runs give the same bits.
//
// NO LANE WAITS FOR ANOTHER.  Every atomic is issued once and its result decides the next step; there are no spins, flags or locks.
// At least half the slots are empty, so a walk ends; its loop is bounded by `slots` all the same, and a lane that used the bound up
// writes nothing.
#include <hip/hip_runtime.h>

#include "../gf2_dev_words.h"
#include "../gf2_kernels.h"
#include "find_plan.h"
#include "gf2_find.h"

namespace {

typedef unsigned long long FindEntry;  // the type of HIP's 64-bit atomics

// ---- a lane per row

// the hash of the columns [c0, c1) of a row.  [w0, w1): the words of a row that hold a column of the range (find_plan.h); no other
// word is read
__device__ __forceinline__ u64 find_row_hash(const u64 *row, long long w0, long long w1, int c0, int c1) {
  u64 acc = 0;
  for (long long k = w0; k < w1; ++k) acc ^= find_word_hash(row[k] & gf2_word_mask(k, c0, c1), k - w0);
  return find_finish(acc);
}

// are two rows equal in every column of [c0, c1)?  No word behind the first that differs is read
__device__ __forceinline__ bool find_rows_equal(const u64 *a, const u64 *b, long long w0, long long w1, int c0, int c1) {
  for (long long k = w0; k < w1; ++k)
    if ((a[k] ^ b[k]) & gf2_word_mask(k, c0, c1)) return false;
  return true;
}

// row j of B goes into the table
__device__ __forceinline__ void find_insert(const u64 *B, long long ldb, long long j, long long w0, long long w1, int c0, int c1,
                                            FindEntry *entries, u64 slots, u32 *counts) {
  const u64 *row = B + j * ldb;
  const u64 hash = find_row_hash(row, w0, w1, c0, c1), mine = find_entry(hash, j);
  u64 s = find_first_slot(hash, slots);
  for (u64 step = 0; step < slots; ++step, s = find_next_slot(s, slots)) {
    u64 v = __atomic_load_n(&entries[s], __ATOMIC_RELAXED);  // a stale value is empty or an equal row above the occupant
    if (v == kFindEmpty) {
      v = atomicCAS(&entries[s], (FindEntry)kFindEmpty, (FindEntry)mine);
      if (v == kFindEmpty) v = mine;  // placed
    }
    if (v != mine) {
      if (find_entry_tag(v) != find_entry_tag(mine) || !find_rows_equal(row, B + find_entry_row(v) * ldb, w0, w1, c0, c1)) continue;
      if (v > mine) atomicMin(&entries[s], (FindEntry)mine);  // the result is not used: the no-return form
    }
    if (counts) atomicAdd(&counts[s], 1u);
    return;
  }
}

// the lowest row of B equal to the row `a` and, in *mult, how many there are: -1 and 0 for none; -2: the bound was used up
__device__ __forceinline__ int find_probe(const u64 *a, const u64 *B, long long ldb, long long w0, long long w1, int c0, int c1,
                                          const FindEntry *entries, u64 slots, const u32 *counts, int *mult) {
  const u64 hash = find_row_hash(a, w0, w1, c0, c1);
  u64 s = find_first_slot(hash, slots);
  *mult = 0;
  for (u64 step = 0; step < slots; ++step, s = find_next_slot(s, slots)) {
    const u64 v = entries[s];
    if (v == kFindEmpty) return -1;
    if (find_entry_tag(v) != find_entry_tag(hash) || !find_rows_equal(a, B + find_entry_row(v) * ldb, w0, w1, c0, c1)) continue;
    if (counts) *mult = (int)counts[s];
    return (int)find_entry_row(v);
  }
  return -2;
}

// ---- a wave per row: lane t takes the words w0 + t, w0 + t + 64, ... of the range; every result is the same in all 64 lanes, and
// lane 0 issues the atomics.  Every lane of the wave calls these

__device__ __forceinline__ u64 find_row_hash_wave(const u64 *row, long long w0, long long w1, int c0, int c1, int lane) {
  u64 acc = 0;
  for (long long k = w0 + lane; k < w1; k += 64) acc ^= find_word_hash(row[k] & gf2_word_mask(k, c0, c1), k - w0);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc ^= __shfl_xor((FindEntry)acc, d, 64);
  return find_finish(acc);
}

// 64 words at a time; nothing behind the 64 words with the first difference is read
__device__ __forceinline__ bool find_rows_equal_wave(const u64 *a, const u64 *b, long long w0, long long w1, int c0, int c1, int lane) {
  for (long long k0 = w0; k0 < w1; k0 += 64) {
    const long long k = k0 + lane;
    const bool differ = k < w1 && ((a[k] ^ b[k]) & gf2_word_mask(k, c0, c1)) != 0;
    if (__any(differ)) return false;
  }
  return true;
}

__device__ __forceinline__ void find_insert_wave(const u64 *B, long long ldb, long long j, long long w0, long long w1, int c0, int c1,
                                                 FindEntry *entries, u64 slots, u32 *counts, int lane) {
  const u64 *row = B + j * ldb;
  const u64 hash = find_row_hash_wave(row, w0, w1, c0, c1, lane), mine = find_entry(hash, j);
  u64 s = find_first_slot(hash, slots);
  for (u64 step = 0; step < slots; ++step, s = find_next_slot(s, slots)) {
    FindEntry v = 0;
    if (lane == 0) {
      v = __atomic_load_n(&entries[s], __ATOMIC_RELAXED);
      if (v == kFindEmpty) {
        v = atomicCAS(&entries[s], (FindEntry)kFindEmpty, (FindEntry)mine);
        if (v == kFindEmpty) v = mine;
      }
    }
    v = __shfl(v, 0, 64);
    if (v != mine) {
      if (find_entry_tag(v) != find_entry_tag(mine) || !find_rows_equal_wave(row, B + find_entry_row(v) * ldb, w0, w1, c0, c1, lane)) continue;
      if (lane == 0 && v > mine) atomicMin(&entries[s], (FindEntry)mine);
    }
    if (lane == 0 && counts) atomicAdd(&counts[s], 1u);
    return;
  }
}

__device__ __forceinline__ int find_probe_wave(const u64 *a, const u64 *B, long long ldb, long long w0, long long w1, int c0, int c1,
                                               const FindEntry *entries, u64 slots, const u32 *counts, int *mult, int lane) {
  const u64 hash = find_row_hash_wave(a, w0, w1, c0, c1, lane);
  u64 s = find_first_slot(hash, slots);
  *mult = 0;
  for (u64 step = 0; step < slots; ++step, s = find_next_slot(s, slots)) {
    const u64 v = entries[s];  // one address for the wave, in a table that the launch only reads
    if (v == kFindEmpty) return -1;
    if (find_entry_tag(v) != find_entry_tag(hash) || !find_rows_equal_wave(a, B + find_entry_row(v) * ldb, w0, w1, c0, c1, lane)) continue;
    if (counts) *mult = (int)counts[s];
    return (int)find_entry_row(v);
  }
  return -2;
}

// ---- kernels

__global__ void __launch_bounds__(kFindThreads) gf2_find_fill_kernel(FindEntry *entries, u32 *counts, u64 slots, int *count) {
  const u64 first = (u64)blockIdx.x * kFindThreads + threadIdx.x;
  for (u64 s = first; s < slots; s += (u64)gridDim.x * kFindThreads) {
    entries[s] = kFindEmpty;
    if (counts) counts[s] = 0;
  }
  if (count && first == 0) *count = 0;
}

template <bool WAVE>
__global__ void __launch_bounds__(kFindThreads) gf2_find_build_kernel(const u64 *B, long long ldb, long long nb, long long w0, long long w1,
                                                                      int c0, int c1, FindEntry *entries, u64 slots, u32 *counts) {
  if (WAVE) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long j0 = ((long long)blockIdx.x * kFindWaves + wave) * kFindWaveRows;
    for (long long j = j0; j < j0 + kFindWaveRows && j < nb; ++j) find_insert_wave(B, ldb, j, w0, w1, c0, c1, entries, slots, counts, lane);
  } else {
    const long long j = (long long)blockIdx.x * kFindThreads + threadIdx.x;
    if (j < nb) find_insert(B, ldb, j, w0, w1, c0, c1, entries, slots, counts);
  }
}

// the hits of a workgroup are summed in LDS -- a ballot's population count per wave -- and go to *count in one atomic
template <bool WAVE>
__global__ void __launch_bounds__(kFindThreads) gf2_find_lookup_kernel(const u64 *A, long long lda, long long na, const u64 *B, long long ldb,
                                                                       long long w0, long long w1, int c0, int c1, const FindEntry *entries,
                                                                       u64 slots, const u32 *counts, int *idx, int *mult, int *count) {
  __shared__ int hits;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) hits = 0;
  __syncthreads();
  if (WAVE) {
    const long long i0 = ((long long)blockIdx.x * kFindWaves + wave) * kFindWaveRows;
    int found = 0;
    for (long long i = i0; i < i0 + kFindWaveRows && i < na; ++i) {
      int m;
      const int r = find_probe_wave(A + i * lda, B, ldb, w0, w1, c0, c1, entries, slots, counts, &m, lane);
      if (lane == 0 && r > -2) {
        idx[i] = r;
        if (mult) mult[i] = m;
      }
      found += r >= 0;
    }
    if (lane == 0 && found) atomicAdd(&hits, found);
  } else {
    const long long i = (long long)blockIdx.x * kFindThreads + threadIdx.x;
    bool found = false;
    if (i < na) {
      int m;
      const int r = find_probe(A + i * lda, B, ldb, w0, w1, c0, c1, entries, slots, counts, &m);
      if (r > -2) {
        idx[i] = r;
        if (mult) mult[i] = m;
      }
      found = r >= 0;
    }
    const u64 bal = __ballot(found);
    if (lane == 0 && bal) atomicAdd(&hits, __popcll(bal));
  }
  __syncthreads();
  if (count && threadIdx.x == 0 && hits) atomicAdd(count, hits);
}

dim3 find_grid(long long items, long long per_group) { return dim3((unsigned)((items + per_group - 1) / per_group)); }  // < 2^26

}  // namespace

extern "C" hipError_t gf2k_find_rows(const u64 *A, long long lda, int nrows_a, const u64 *B, long long ldb, int nrows_b, int c0, int c1,
                                     void *table, int *idx, int *mult, int *count, hipStream_t stream) {
  const FindPlan plan = find_plan(nrows_a, nrows_b, c1, c0, c1);
  if (plan.slots <= 0 || nrows_a <= 0) return hipErrorInvalidValue;
  const u64 slots = (u64)plan.slots;
  FindEntry *entries = static_cast<FindEntry *>(table);
  u32 *counts = mult ? reinterpret_cast<u32 *>(static_cast<char *>(table) + plan.entry_bytes) : nullptr;
  const long long w0 = find_first_word(c0, c1), w1 = find_end_word(c0, c1), fill = (plan.slots + kFindThreads - 1) / kFindThreads;
  const dim3 block(kFindThreads);
  hipLaunchKernelGGL(gf2_find_fill_kernel, dim3((unsigned)(fill < kFindFillMaxGroups ? fill : kFindFillMaxGroups)), block, 0, stream, entries,
                     counts, slots, count);
  if (plan.wave) {
    hipLaunchKernelGGL((gf2_find_build_kernel<true>), find_grid(nrows_b, plan.build_rows), block, 0, stream, B, ldb, (long long)nrows_b, w0, w1,
                       c0, c1, entries, slots, counts);
    hipLaunchKernelGGL((gf2_find_lookup_kernel<true>), find_grid(nrows_a, plan.lookup_rows), block, 0, stream, A, lda, (long long)nrows_a, B, ldb,
                       w0, w1, c0, c1, (const FindEntry *)entries, slots, (const u32 *)counts, idx, mult, count);
  } else {
    hipLaunchKernelGGL((gf2_find_build_kernel<false>), find_grid(nrows_b, plan.build_rows), block, 0, stream, B, ldb, (long long)nrows_b, w0, w1,
                       c0, c1, entries, slots, counts);
    hipLaunchKernelGGL((gf2_find_lookup_kernel<false>), find_grid(nrows_a, plan.lookup_rows), block, 0, stream, A, lda, (long long)nrows_a, B,
                       ldb, w0, w1, c0, c1, (const FindEntry *)entries, slots, (const u32 *)counts, idx, mult, count);
  }
  return hipGetLastError();
}
