// gf2_lpn.inc -- single-phase streaming kernels for batches of LPN-style products (BASELINE config 5):
// C (m x n) = A (m x l) * B (l x n) with l <= 256 and n <= 256, m large.  mzd_mul_naive as `mul_slice` / `&A * &v` reach it
// (m4ri-rust's BinMatrix::mul_slice and its `*` operators).
// Included by gf2_kernels.hip (the product: launched by gf2k_tallskinny there) and by tools/lpn_lab.hip
// (development harness); needs u32 / u64, the lds_* typedefs, xor4 and static_for.
//
// Both kernels keep the Four-Russians tables of ALL 256 bits of the inner dimension resident in LDS, built once per workgroup,
// and stream the rows of A through them: a lane owns a whole 32-byte row, looks its fields up, stores its row of C and goes on
// to the next row with the loads of later rows in flight -- reads and writes overlap for the whole launch, every byte moves once.
// Conflict-free lookups whatever the entries are come from the skewed layout of gf2_tallskinny3/5_kernel: a 256-byte LDS row
// holds entry e of several tables side by side, and the lanes that the LDS serves together visit those tables in different
// orders (table = step ^ lane bits), which costs a per-lane XOR-permutation of the row's dwords / bytes once per row.
//
// MODE: 0 = any strides, l <= 256 (8-byte loads, masks); 1 = rows of A 16-byte aligned, l > 192 (two 16-byte loads per lane);
// 2 = A contiguous (lda == 4 words): a wave's 64 rows are 2 KiB of consecutive bytes, fetched by two wave-contiguous 16-byte
// loads (lane j and lane j + 32 take the two halves of row j, then of row 32 + j) and handed to their owners by four
// v_permlane32_swap_b32 -- a lane-per-row load touches every 128-byte line of the 2 KiB twice, 16 bytes in 32, and a plain stream
// of this shape measured 14.5 us where the contiguous one takes 12.3 (tools/lpn_lab, 2^20 rows, 32 bytes in and out per row).
// Loads of A and stores of C are non-temporal: each byte is touched once.

// per-lane choice between two registers with ONE VALU instruction: mask all ones -> b, zero -> a (written out because the
// compiler turns `flag ? q[i ^ 2] : q[i]` into an indexed select: seven compare / v_cndmask pairs per element)
__device__ __forceinline__ u32 lpn_pick(u32 a, u32 b, u32 mask) {
  u32 r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xd8" : "=v"(r) : "v"(a), "v"(b), "v"(mask));
  return r;
}
// lanes 32-63 of a <-> lanes 0-31 of b (four of these turn two wave-contiguous 16-byte loads into one 32-byte row per lane)
// (The builtin, not inline asm: a VALU write of either operand needs two wait states before the swap reads it, and the compiler
// only pads what it can see -- the transposition's asm form of the 16-lane swap read a stale register, round 4.)
__device__ __forceinline__ void lpn_swap32(u32x4 &a, u32x4 &b) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto r = __builtin_amdgcn_permlane32_swap(a[i], b[i], false, false);
    a[i] = r[0], b[i] = r[1];
  }
}

// The loads of one row per lane (64 rows per wave), issued now and completed (swapped / unpacked) when the row is used.
//   h = 1: the lane wants the upper 16 bytes of its row in d[0..3] (a skew bit applied by the addresses: free)
template <int MODE>
struct lpn_row_loader {
  u32x4 x, y;
  __device__ __forceinline__ void issue(const u64 *__restrict__ A, long long lda, long long wave_row, int lane, int h, int m, int l) {
    if constexpr (MODE == 2) {
      const u32x4 *a4 = reinterpret_cast<const u32x4 *>(A);
      const long long p = wave_row * 2 + 2 * (lane & 31) + (h ^ (lane >> 5)), pmax = (long long)m * 2 - 1;
      x = __builtin_nontemporal_load(a4 + min(p, pmax));
      y = __builtin_nontemporal_load(a4 + min(p + 64, pmax));
    } else {
      const long long row = min(wave_row + lane, (long long)m - 1);  // clamped: stores are guarded
      const u64 *ap = A + row * lda;
      if constexpr (MODE == 1) {
        const u32x4 *ap4 = reinterpret_cast<const u32x4 *>(__builtin_assume_aligned(ap, 16));
        x = __builtin_nontemporal_load(ap4 + h);
        y = __builtin_nontemporal_load(ap4 + (h ^ 1));
      } else {
        const int wl = (l + 63) >> 6;
        u64 w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = (q ^ (2 * h)) < wl ? ap[min(q ^ (2 * h), wl - 1)] : 0;  // (bits past l meet zero rows of B)
        x.x = (u32)w[0], x.y = (u32)(w[0] >> 32), x.z = (u32)w[1], x.w = (u32)(w[1] >> 32);
        y.x = (u32)w[2], y.y = (u32)(w[2] >> 32), y.z = (u32)w[3], y.w = (u32)(w[3] >> 32);
      }
    }
  }
  __device__ __forceinline__ void finish(u32 (&d)[8]) {
    if constexpr (MODE == 2) lpn_swap32(x, y);
    d[0] = x.x, d[1] = x.y, d[2] = x.z, d[3] = x.w, d[4] = y.x, d[5] = y.y, d[6] = y.z, d[7] = y.w;
  }
};

// ---------------------------------------------------------------------------------------------
// n <= 128: 8-bit tables of 8 NW-byte entries (NW = 1, 2 words per row of C), 32 / NW tables per 256-byte LDS row: 64 KiB per
// 32 / NW bytes of a row ("row set": NW = 1 has one, NW = 2 two).  A ds_read_b64 serves 32 lanes per cycle, a ds_read_b128 16
// (bank = (address / 4) mod 64), so lane L reads table c ^ (L mod 32 / NW) at step c: 32 / NW different slots of 8 NW bytes.
// Per row: 2 loads, 8 v_perm + 8 selects (the permutation; NW = 1 applies its fifth skew bit by the order of the two loads),
// 32 x (v_perm for the address, one LDS read, v_bitop3 per dword and pair of lookups) -- ~125 (NW = 1) / ~160 (NW = 2) VALU + LDS
// instructions against ~300 for the 4-bit kernel (gf2_tallskinny6_kernel).
// ABL (tools/lpn_lab only, wrong results by design): 1 = no table build, 2 = no lookups.
// ---------------------------------------------------------------------------------------------
constexpr int kLpn8LdsBytes(int nw) { return 65536 * nw + 32 * (64 * nw + 16); }  // tables + the staged rows of B

template <int NW, int NT, int RPT, int MODE, int EARLY = (RPT < 2 ? RPT : 2), int ABL = 0, int STRIDED = 0>
__global__ __launch_bounds__(NT) void gf2_lpn8_kernel(const u64 *__restrict__ A, long long lda, const u64 *__restrict__ B,
                                                      long long ldb, u64 *__restrict__ C, long long ldc, int m, int l, int n,
                                                      int accumulate) {
  extern __shared__ __align__(16) unsigned char lds[];
  static_assert(NW == 1 || NW == 2, "entries of 8 or 16 bytes");
  static_assert(NT == 256 || NT == 512 || NT == 1024, "build items = 32 tables x NT / 32 high parts");
  constexpr int HB = NT == 256 ? 3 : NT == 512 ? 4 : 5;  // high bits of an entry index fixed per build item
  constexpr int GB = 8 - HB;                            // low bits walked in Gray-code order
  constexpr int TPR = 32 / NW;                          // tables per LDS row = steps per row set
  const int tid = threadIdx.x, lane = tid & 63, s = lane & (TPR - 1);
  const int wn = (n + 63) >> 6;
  const u64 maskC = (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;

  // ---- B first (in-order return: the build waits for it alone): 256 rows x NW words, one word per thread, staged in LDS behind
  // the tables.  (Each thread fetching the eight rows of its own table straight from global memory -- lanes 128 bytes apart, 32
  // lines per instruction -- cost 0.9 us at NW = 1 and 5 us at NW = 2.)  The 8 rows of table t lie at t * (64 NW + 16) bytes:
  // with that pitch the 16-byte reads of the build are conflict-free ----
  constexpr int PITCH = 64 * NW + 16;
  const int t = tid & 31, hi = tid >> 5;
  u64 bword = 0;
  if (tid < 256 * NW) {
    const int row = tid / NW, w = tid % NW;
    bword = B[(long long)min(row, l - 1) * ldb + min(w, wn - 1)] & (0ull - (u64)(row < l && w < wn));
    if (w == wn - 1) bword &= maskC;  // (excess bits of B are zero by M4RI's invariant; masked here so that no store has to)
  }
  // ---- rows of A: NT consecutive rows per step, 64 per wave; NW = 1: a row's 16-byte halves in the order of skew bit 4 ----
  static_assert(EARLY >= 1 && EARLY <= RPT, "rows requested ahead");
  // STRIDED: row steps in grid-stride order -- step r of workgroup b takes rows (r * gridDim.x + b) * NT ... -- so that at any time the
  // launch reads ONE contiguous window of A and writes one of C, as a plain stream does, instead of gridDim.x places NT * RPT rows apart
  const long long step_rows = STRIDED ? (long long)gridDim.x * NT : (long long)NT;
  const long long wave_row0 = (STRIDED ? (long long)blockIdx.x * NT : (long long)blockIdx.x * (NT * RPT)) + (tid & ~63);
  const int h0 = NW == 1 ? (s >> 4) & 1 : 0;
  lpn_row_loader<MODE> ld[RPT];
#pragma unroll
  for (int r = 0; r < EARLY; ++r) ld[r].issue(A, lda, wave_row0 + (long long)r * step_rows, lane, h0, m, l);

  if (tid < 256 * NW) {
    const int row = tid / NW, w = tid % NW;
    *reinterpret_cast<u64 *>(lds + 65536 * NW + (row >> 3) * PITCH + (row & 7) * (8 * NW) + 8 * w) = bword;
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  // ---- build: entry e of table t at (t / TPR) * 65536 + e * 256 + (t % TPR) * 8 NW ----
  if constexpr (!(ABL & 1)) {
    u64 br[8][NW];
    {
      const uint4 *src = reinterpret_cast<const uint4 *>(lds + 65536 * NW + t * PITCH);
#pragma unroll
      for (int k = 0; k < 4 * NW; ++k) {
        const uint4 x = src[k];  // bytes 16 k .. 16 k + 15 of the 8 rows (8 NW bytes each)
        const u64 lo = (u64)x.x | ((u64)x.y << 32), hi64 = (u64)x.z | ((u64)x.w << 32);
        br[(2 * k) / NW][(2 * k) % NW] = lo;
        br[(2 * k + 1) / NW][(2 * k + 1) % NW] = hi64;
      }
    }
    u64 v[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      v[w] = 0;
#pragma unroll
      for (int b = 0; b < HB; ++b) v[w] ^= br[GB + b][w] & (0ull - (u64)((hi >> b) & 1));
    }
    unsigned char *tb = lds + (t / TPR) * 65536 + (t % TPR) * (8 * NW) + (hi << GB) * 256;
#pragma unroll
    for (int i = 0; i < (1 << GB); ++i) {
      const int gc = i ^ (i >> 1);
      if (i) {
#pragma unroll
        for (int w = 0; w < NW; ++w) v[w] ^= br[__builtin_ctz(i)][w];
      }
      u64 *dst = reinterpret_cast<u64 *>(tb + gc * 256);
#pragma unroll
      for (int w = 0; w < NW; ++w) dst[w] = v[w];
    }
  }
  // per-lane constants: byte permutation y -> y ^ (s & 3), taken from the partner dword when skew bit 2 is set
  const u32 bsel0 = (s & 3) == 0 ? 0x03020100u : (s & 3) == 1 ? 0x02030001u : (s & 3) == 2 ? 0x01000302u : 0x00010203u;
  const u32 bsel = bsel0 | ((s & 4) ? 0x04040404u : 0u);
  const u32 sw8 = 0u - (u32)((s >> 3) & 1);
  // address bytes of the steps, packed: NW = 1: byte i of X[j] = ((4 j + i) ^ s) * 8 (step 4 j + i);
  // NW = 2: bytes 0, 1 of X[j] = ((2 j + i) mod 16 ^ s) * 16 for steps 2 j, 2 j + 1 of a row set, byte 2 = the row set (64 KiB each)
  u32 X[NW == 1 ? 8 : 16];
  if constexpr (NW == 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      u32 x = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) x |= (u32)((((4 * j + i) ^ s) * 8) & 0xff) << (8 * i);
      X[j] = x;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      u32 x = (u32)(j >> 3) << 16;
#pragma unroll
      for (int i = 0; i < 2; ++i) x |= (u32)(((((2 * j + i) & 15) ^ s) * 16) & 0xff) << (8 * i);
      X[j] = x;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    __builtin_amdgcn_sched_barrier(0);
    if (r + EARLY < RPT) ld[r + EARLY].issue(A, lda, wave_row0 + (long long)(r + EARLY) * step_rows, lane, h0, m, l);
    __builtin_amdgcn_sched_barrier(0);
    u32 d[8], q[8], dp[8];
    ld[r].finish(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = __builtin_amdgcn_perm(d[i ^ 1], d[i], bsel);
#pragma unroll
    for (int i = 0; i < 8; ++i) dp[i] = lpn_pick(q[i], q[i ^ 2], sw8);
    u32 acc[2 * NW];
#pragma unroll
    for (int i = 0; i < 2 * NW; ++i) acc[i] = 0;
    if constexpr (ABL & 2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i % (2 * NW)] ^= dp[i];
    } else if constexpr (NW == 1) {
#pragma unroll
      for (int c = 0; c < 32; c += 2) {
        const u32 o0 = __builtin_amdgcn_perm(dp[c >> 2], X[c >> 2], 0x0c0c0000u | ((4u + (c & 3)) << 8) | (u32)(c & 3));
        const u32 o1 = __builtin_amdgcn_perm(dp[(c + 1) >> 2], X[(c + 1) >> 2], 0x0c0c0000u | ((4u + ((c + 1) & 3)) << 8) | (u32)((c + 1) & 3));
        const u32x2v x = *reinterpret_cast<lds_cu32x2 *>(o0), y = *reinterpret_cast<lds_cu32x2 *>(o1);
        asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[0]) : "v"(x.x), "v"(y.x));
        asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[1]) : "v"(x.y), "v"(y.y));
      }
    } else {
#pragma unroll
      for (int c = 0; c < 32; c += 2) {  // byte c of the permuted row: row set c / 16, step c % 16
        const u32 o0 = __builtin_amdgcn_perm(dp[c >> 2], X[c >> 1], 0x0c020000u | ((4u + (c & 3)) << 8) | 0u);
        const u32 o1 = __builtin_amdgcn_perm(dp[(c + 1) >> 2], X[c >> 1], 0x0c020000u | ((4u + ((c + 1) & 3)) << 8) | 1u);
        const u32x4 x = *reinterpret_cast<lds_cu32x4 *>(o0), y = *reinterpret_cast<lds_cu32x4 *>(o1);
        asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[0]) : "v"(x.x), "v"(y.x));
        asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[1]) : "v"(x.y), "v"(y.y));
        asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[2]) : "v"(x.z), "v"(y.z));
        asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[3]) : "v"(x.w), "v"(y.w));
      }
    }
    const long long row = wave_row0 + (long long)r * step_rows + lane;
    if (row < m) {
      if constexpr (NW == 1) {
        u64 v = (u64)acc[0] | ((u64)acc[1] << 32);
        u64 *dd = C + row * ldc;
        if (accumulate) v ^= *dd;
        __builtin_nontemporal_store(v, dd);
      } else {
        u64 *dd = C + row * ldc;
        if (MODE >= 1 && wn == 2 && (ldc & 1) == 0) {  // (MODE >= 1 also says: C 16-byte aligned)
          u32x4 v;
          v.x = acc[0], v.y = acc[1], v.z = acc[2], v.w = acc[3];
          u32x4 *d4 = reinterpret_cast<u32x4 *>(__builtin_assume_aligned(dd, 16));
          if (accumulate) v ^= *d4;
          __builtin_nontemporal_store(v, d4);
        } else {
#pragma unroll
          for (int w = 0; w < NW; ++w)
            if (w < wn) {
              u64 v = (u64)acc[2 * w] | ((u64)acc[2 * w + 1] << 32);
              if (accumulate) v ^= dd[w];
              dd[w] = v;
            }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// n <= 4 (`&A * &v`, mul_slice, binary_matrix.rs:416-431: ONE vector is the reference's own operator): no tables at all.  Column j of
// B is 256 bits = 8 dwords, wave-uniform: lane k reads rows k, k + 64, k + 128, k + 192 of B and four ballots per vector put it
// into scalar registers; a row of A (the same wave-contiguous loads as above) then costs 8 x v_bitop3 ((a & b) ^ c) and one
// v_bcnt per vector.  What the table kernels pay before their first lookup -- B staged, 64 KiB of tables built, two barriers:
// ~1.5 us of the 8.8 us a 2^20-row product takes -- is gone: every load of a workgroup's rows is in flight before B is even
// requested (2^20 x 256 x 1: cold 9.0 -> 8.5 us, which is 4.9 TB/s of the 41.9 MB that move -- the cold stream's own rate at this size --, warm 7.5 -> 5.7 us).
// ---------------------------------------------------------------------------------------------
template <int NV, int NT, int RPT, int MODE, int STRIDED = 0>
__global__ __launch_bounds__(NT) void gf2_lpnvec_kernel(const u64 *__restrict__ A, long long lda, const u64 *__restrict__ B,
                                                        long long ldb, u64 *__restrict__ C, long long ldc, int m, int l, int n,
                                                        int accumulate, u64 *__restrict__ side, long long side_ld) {
  static_assert(NV >= 1 && NV <= 4, "vectors in scalar registers: 8 per vector");
  const int tid = threadIdx.x, lane = tid & 63;
  const long long step_rows = STRIDED ? (long long)gridDim.x * NT : (long long)NT;  // (grid-stride row steps, see gf2_lpn8_kernel)
  const long long wave_row0 = (STRIDED ? (long long)blockIdx.x * NT : (long long)blockIdx.x * (NT * RPT)) + (tid & ~63);
  lpn_row_loader<MODE> ld[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) ld[r].issue(A, lda, wave_row0 + (long long)r * step_rows, lane, 0, m, l);
  u64 bw[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = 64 * q + lane;
    bw[q] = B[(long long)min(row, l - 1) * ldb] & (0ull - (u64)(row < l));  // (bits of A past l meet zero)
  }
  u32 vs[NV][8];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u64 bal = j < n ? __ballot((int)((bw[q] >> j) & 1)) : 0ull;
      vs[j][2 * q] = (u32)bal, vs[j][2 * q + 1] = (u32)(bal >> 32);
    }
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    u32 d[8];
    ld[r].finish(d);
    u64 v = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      u32 t = d[0] & vs[j][0];
#pragma unroll
      for (int i = 1; i < 8; ++i) t = __builtin_amdgcn_bitop3_b32(d[i], vs[j][i], t, 0x6a);  // (d & v) ^ t
      v |= (u64)(__builtin_popcount(t) & 1) << j;
    }
    const long long row = wave_row0 + (long long)r * step_rows + lane;
    if (row < m) {
      u64 *dd = C + row * ldc;
      if (accumulate) v ^= *dd;
      __builtin_nontemporal_store(v, dd);
    }
    // the packed transposed form beside C (round 5: what `as_vector` of `&A * &v` asks for next, binary_matrix.rs:332-361): a lane
    // holds the results of ITS row, so bit j of the wave's 64 rows is one ballot (rows past m contribute zeros)
    if (side) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const u64 bal = __ballot((int)((v >> j) & 1) && row < m);
        if (lane == 0 && j < n && row < m) side[(long long)j * side_ld + (row >> 6)] = bal;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 128 < n <= 256: 32-byte entries.  8-bit tables of all 256 bits would take 256 KiB, so gf2_tallskinny5_kernel<4> runs two
// phases (tables of 128 bits at a time) and keeps loads and stores apart.  Here every dword of a row is cut into FIVE fields of
// 6 + 6 + 6 + 7 + 7 bits instead of four bytes: 448 entries per dword, 8 x 448 x 32 B = 112 KiB for the whole inner dimension --
// one phase, 40 lookups per row instead of 32.  Group j (field j of every dword) is an array of 256-byte LDS rows, row e = entry
// e of the eight tables (dword 0..7, 32 bytes each); a ds_read_b128 serves 16 lanes per cycle, lane L visits the dwords in the
// order c ^ (L & 7) and reads the 16-byte halves of an entry in the order given by lane bit 3: sixteen different 16-byte slots.
// Addresses: field << 8 | slot, formed by full-rate VOP2 instructions; the groups' bases are instruction immediates (the last
// group lies beyond the 64 KiB an immediate reaches: its slot constants carry bit 16).
// MODE 2 also stores C (ldc == 4) wave-contiguously, through the same swap as the loads.
// ---------------------------------------------------------------------------------------------
#ifdef GF2_LPN_LAB
__device__ unsigned long long *lpn_dbg_stamps;  // tools/lpn_lab: 16 u64 per wave when ABL & 4
#define LPN_STAMP(k, expr)                                                                   \
  do {                                                                                       \
    if constexpr ((ABL & 12) != 0) {                                                         \
      if (lane == 0) lpn_dbg_stamps[((long long)blockIdx.x * (NT / 64) + (tid >> 6)) * 16 + (k)] = (expr); \
    }                                                                                        \
  } while (0)
#else
#define LPN_STAMP(k, expr) do { } while (0)
#endif
__device__ constexpr int kLpnFieldPos[5] = {0, 6, 12, 18, 25};
__device__ constexpr int kLpnFieldBits[5] = {6, 6, 6, 7, 7};
__device__ constexpr int kLpnGroupBase[5] = {0, 16384, 32768, 49152, 81920};
constexpr int kLpn256TableBytes = 114688;  // 112 KiB
constexpr int kLpn256LdsBytes = kLpn256TableBytes + 264 * 32;  // + the 256 rows of B, one 32-byte pad per 32 rows (see the build)

template <int NT, int RPT, int MODE, int EARLY = (RPT < 2 ? RPT : 2), int ABL = 0, int ORD = 0>
__global__ __launch_bounds__(NT) void gf2_lpn256_kernel(const u64 *__restrict__ A, long long lda, const u64 *__restrict__ B,
                                                        long long ldb, u64 *__restrict__ C, long long ldc, int m, int l, int n,
                                                        int accumulate) {
  extern __shared__ __align__(16) unsigned char lds[];
  static_assert(NT == 1024 || NT == 512, "the staging of B and the build are written for 1024 / NT passes");
  constexpr int PASSES = 1024 / NT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int s3 = lane & 7, hsw = (lane >> 3) & 1;
  const int wn = (n + 63) >> 6;
  const u64 maskC = (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;

  LPN_STAMP(0, __builtin_amdgcn_s_memrealtime());
  LPN_STAMP(1, __builtin_amdgcn_s_memtime());
  // ---- B first: 256 rows x 4 words, one word per thread (rows past l and words past n are zero) ----
  u64 bword[PASSES];
#pragma unroll
  for (int ps = 0; ps < PASSES; ++ps) {
    const int idx = tid + ps * NT, brow = idx >> 2, w = idx & 3;
    bword[ps] = B[(long long)min(brow, l - 1) * ldb + min(w, wn - 1)] & (0ull - (u64)(brow < l && w < wn));
    if (w == wn - 1) bword[ps] &= maskC;  // (excess bits of B are zero by M4RI's invariant; masked here so that no store has to)
  }
  // ---- rows of A ----
  static_assert(EARLY >= 1 && EARLY <= RPT, "rows requested ahead");
  // ORD & 8: row steps in grid-stride order (step r of workgroup b = rows (r * gridDim.x + b) * NT ...): at any time the launch reads ONE
  // contiguous window of A and writes one of C, as a plain stream does, instead of 256 places 128 KiB apart
  const long long step_rows = (ORD & 8) ? (long long)gridDim.x * NT : (long long)NT;
  const long long wave_row0 = ((ORD & 8) ? (long long)blockIdx.x * NT : (long long)blockIdx.x * (NT * RPT)) + (tid & ~63);
  const int h0 = (s3 >> 2) & 1;
  lpn_row_loader<MODE> ld[RPT];
  if constexpr (!(ORD & 4)) {
#pragma unroll
    for (int r = 0; r < EARLY; ++r) ld[r].issue(A, lda, wave_row0 + (long long)r * step_rows, lane, h0, m, l);
  }

  // staged with a pad of 32 bytes per 32 rows: the build's lanes w = 0..7 read rows 32 w + k together, which would otherwise
  // share their banks (SQ_LDS_BANK_CONFLICT: 22 % of the kernel's LDS cycles in the first version)
  u64 *bst = reinterpret_cast<u64 *>(lds + kLpn256TableBytes);
#pragma unroll
  for (int ps = 0; ps < PASSES; ++ps) {
    const int idx = tid + ps * NT;
    bst[idx + ((idx >> 7) << 2)] = bword[ps];
  }
  if constexpr ((ORD & 4) != 0) {  // (variant: the rows of A requested only once B has arrived)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < EARLY; ++r) ld[r].issue(A, lda, wave_row0 + (long long)r * step_rows, lane, h0, m, l);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  LPN_STAMP(2, __builtin_amdgcn_s_memtime());

  // ---- build, 16 waves: a 256-byte LDS row (entry e of the eight tables of a group) is ONE ds_write_addtid_b32 (address = M0 + offset +
  // 4 lane: 256 bytes in 2 LDS cycles, against ~13 for the same bytes by ds_write_b128).  Lane (w = lane / 8, k = lane % 8) holds
  // dword k of dword w's entry; a wave takes blocks of 16 consecutive entries (28 blocks in all), starts a block from the rows
  // of its high bits and walks the low four bits in Gray-code order: one v_xor_b32 and one write per entry.  (The first version --
  // a run of four entries per thread, 16-byte reads and writes -- took 3900 cycles of the kernel's ~40000; in-kernel stamps.)
  if constexpr (!(ABL & 1) && NT == 1024) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bw = lane >> 3, bk = lane & 7;
    int nblk = 0;
    for (int blk = wave; blk < 28; blk += NT / 64, ++nblk) {  // (uniform)
      const int j = blk < 12 ? blk >> 2 : 3 + ((blk - 12) >> 3), hb = blk < 12 ? blk & 3 : (blk - 12) & 7;
      const int pos = j == 0 ? 0 : j == 1 ? 6 : j == 2 ? 12 : j == 3 ? 18 : 25;
      const u32 base = (u32)(j == 0 ? 0 : j == 1 ? 16384 : j == 2 ? 32768 : j == 3 ? 49152 : 81920) + (u32)hb * 4096u;
      const u32 *rows = reinterpret_cast<const u32 *>(bst) + (33 * bw + pos) * 8 + bk;  // dword bk of row 32 bw + pos (+ 8 per row)
      const u32 r0 = rows[0], r1 = rows[8], r2 = rows[16], r3 = rows[24];
      u32 v = (rows[32] & (0u - (u32)(hb & 1))) ^ (rows[40] & (0u - (u32)((hb >> 1) & 1))) ^ (rows[48] & (0u - (u32)((hb >> 2) & 1)));
      // entries base + Gray(i), i = 0..15: flip bit ctz(i) before write i.  M0 holds at most 0xFFFC and the offset 16 bits: blocks
      // beyond 64 KiB put 48 KiB into the offset.  (s_nop: SALU write of M0 -> add-tid LDS instruction needs a wait state.)
      // Four value registers in rotation: a store reads its data register some time after issue, and overwriting the register
      // right behind the store stalls the wave until it has (a single register: 65 cycles per entry; stamps).
#define LPN_W(K, E, V) "ds_write_addtid_b32 %" #V " offset:" #K "+" #E "*256\n\t"
#define LPN_X(D, S, R) "v_xor_b32 %" #D ", %" #S ", %" #R "\n\t"
#define LPN_GRAY16(K)                                                                                                          \
  asm volatile("s_mov_b32 m0, %8\n\ts_nop 0\n\t"                                                                           \
               LPN_W(K, 0, 0) LPN_X(1, 0, 4) LPN_W(K, 1, 1) LPN_X(2, 1, 5) LPN_W(K, 3, 2) LPN_X(3, 2, 4) LPN_W(K, 2, 3)          \
               LPN_X(0, 3, 6) LPN_W(K, 6, 0) LPN_X(1, 0, 4) LPN_W(K, 7, 1) LPN_X(2, 1, 5) LPN_W(K, 5, 2) LPN_X(3, 2, 4) LPN_W(K, 4, 3) \
               LPN_X(0, 3, 7) LPN_W(K, 12, 0) LPN_X(1, 0, 4) LPN_W(K, 13, 1) LPN_X(2, 1, 5) LPN_W(K, 15, 2) LPN_X(3, 2, 4) LPN_W(K, 14, 3) \
               LPN_X(0, 3, 6) LPN_W(K, 10, 0) LPN_X(1, 0, 4) LPN_W(K, 11, 1) LPN_X(2, 1, 5) LPN_W(K, 9, 2) LPN_X(3, 2, 4)          \
               "ds_write_addtid_b32 %3 offset:" #K "+8*256"                                                                    \
               : "+v"(v), "=&v"(t1), "=&v"(t2), "=&v"(t3) : "v"(r0), "v"(r1), "v"(r2), "v"(r3), "s"(m0v) : "memory")
      u32 t1, t2, t3;
      if (base >= 65536u) {
        const u32 m0v = base - 49152u;
        LPN_GRAY16(49152);
      } else {
        const u32 m0v = base;
        LPN_GRAY16(0);
      }
#undef LPN_GRAY16
#undef LPN_X
#undef LPN_W
    }
  }
  // ---- build, 8 waves: few, wide LDS instructions -- a wave issues one LDS instruction per ~35-45 cycles however little it carries, and
  // with 8 waves that, not the LDS bandwidth, is what a build costs (per-wave stamps: 3600-3900 cycles for 16-byte runs of four
  // entries per thread as for one ds_write_addtid_b32 per table row; this form: 16 ds_write_b128 + 7 ds_read_b128 per wave; the same build
  // with 8-byte writes -- 32 ds_write_b64 per wave, units of 32 entries over all 8 waves -- measured 4200 cycles against 3500, 18.45 us
  // against 17.47 for the product: the instruction count, not the width, is what the build pays for).
  // A wave takes a block of 64 entries of a group (7 blocks: groups 0-2 whole, groups 3 and 4 in two halves): lane
  // (g = lane / 16, w = lane / 2 % 8, half = lane % 2) holds 16 bytes of dword w's entry, bits 4-5 of the entry index = g (and bit 6
  // = the block's half), and walks the low four bits in Gray-code order: four v_xor_b32 and one 16-byte write per step, the
  // write covering FOUR 256-byte table rows ----
  if constexpr (!(ABL & 1) && NT != 1024) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bg = lane >> 4, bw = (lane >> 1) & 7, bhalf = lane & 1;
    for (int blk = wave; blk < 7; blk += NT / 64) {  // (uniform)
      const int j = blk < 3 ? blk : 3 + ((blk - 3) >> 1), hb = blk < 3 ? 0 : (blk - 3) & 1;
      const int pos = j == 0 ? 0 : j == 1 ? 6 : j == 2 ? 12 : j == 3 ? 18 : 25;
      const int gbase = j == 0 ? 0 : j == 1 ? 16384 : j == 2 ? 32768 : j == 3 ? 49152 : 81920;
      const uint4 *rows = reinterpret_cast<const uint4 *>(bst) + (33 * bw + pos) * 2 + bhalf;  // this half of row 32 w + pos (+ 2 per row)
      const uint4 r0 = rows[0], r1 = rows[2], r2 = rows[4], r3 = rows[6], r4 = rows[8], r5 = rows[10], r6 = rows[12];
      const u32 m4 = 0u - (u32)(bg & 1), m5 = 0u - (u32)(bg >> 1), m6 = 0u - (u32)hb;
      uint4 va = make_uint4((r4.x & m4) ^ (r5.x & m5) ^ (r6.x & m6), (r4.y & m4) ^ (r5.y & m5) ^ (r6.y & m6),
                            (r4.z & m4) ^ (r5.z & m5) ^ (r6.z & m6), (r4.w & m4) ^ (r5.w & m5) ^ (r6.w & m6)), vb;
      unsigned char *dst = lds + gbase + ((hb << 6) | (bg << 4)) * 256 + (lane & 15) * 16;
      auto put = [&](int e, const uint4 &v) __attribute__((always_inline)) { *reinterpret_cast<uint4 *>(dst + e * 256) = v; };
      // Gray code over bits 0-3: entry index after step i = i ^ (i >> 1), the bit flipped before it = ctz(i); two value
      // registers in turn (a store reads its data some time after issue)
      put(0, va);
      vb = xor4(va, r0), put(1, vb);
      va = xor4(vb, r1), put(3, va);
      vb = xor4(va, r0), put(2, vb);
      va = xor4(vb, r2), put(6, va);
      vb = xor4(va, r0), put(7, vb);
      va = xor4(vb, r1), put(5, va);
      vb = xor4(va, r0), put(4, vb);
      va = xor4(vb, r3), put(12, va);
      vb = xor4(va, r0), put(13, vb);
      va = xor4(vb, r1), put(15, va);
      vb = xor4(va, r0), put(14, vb);
      va = xor4(vb, r2), put(10, va);
      vb = xor4(va, r0), put(11, vb);
      va = xor4(vb, r1), put(9, va);
      vb = xor4(va, r0), put(8, vb);
    }
  }
  // per-lane constants: low address byte of step c for the half read first
  u32 xa[8], xah[8];  // (xah: the last group lies beyond the 64 KiB an immediate reaches)
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    xa[c] = (u32)(((c ^ s3) * 32) | (hsw * 16));
    xah[c] = xa[c] | 65536u;
  }
  const u32 sw1 = 0u - (u32)(s3 & 1), sw2 = 0u - (u32)((s3 >> 1) & 1);
  LPN_STAMP(3, __builtin_amdgcn_s_memtime());
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  LPN_STAMP(4, __builtin_amdgcn_s_memtime());

#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    __builtin_amdgcn_sched_barrier(0);
    if (r + EARLY < RPT) ld[r + EARLY].issue(A, lda, wave_row0 + (long long)(r + EARLY) * step_rows, lane, h0, m, l);
    __builtin_amdgcn_sched_barrier(0);
    u32 d[8], q[8], dp[8];
    ld[r].finish(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = lpn_pick(d[i], d[i ^ 1], sw1);
#pragma unroll
    for (int i = 0; i < 8; ++i) dp[i] = lpn_pick(q[i], q[i ^ 2], sw2);
    u32 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0;
    // 20 pairs of lookups through a three-stage pipeline: the reads of pair p + 2 are issued before pair p is folded in, so
    // eight ds_read_b128 are in flight behind every wait (the compiler left to itself waits for each pair before the next)
    u32x4 bl[3][2], bh[3][2];
    auto issue = [&dp, &xa, &xah, &bl, &bh](auto P, auto ST) __attribute__((always_inline)) {
      constexpr int p = decltype(P)::value, st = decltype(ST)::value;
      constexpr int L0 = 2 * p, L1 = 2 * p + 1, c0 = L0 / 5, j0 = L0 % 5, c1 = L1 / 5, j1 = L1 % 5;
      // field << 8 | slot by a shift and one v_bitop3_b32 (tools/ubench puts v_bfe_u32 / v_lshl_or_b32 / v_and_or_b32 at half
      // rate, shifts and v_bitop3_b32 near full rate; the mask in an SGPR: VOP3 takes no literal on gfx9); the second half's
      // address is the first's with bit 4 flipped.  ONE asm block for the pair, the two lookups interleaved: between separate
      // asm statements the compiler pads every dependent pair with an s_nop (it cannot see what the instructions are).
      // v_lshlrev_b32 with a negative count is not generated: a right shift by -sh is v_lshrrev_b32
      u32 oa0, ob0, oa1, ob1;
      constexpr int sh0 = 8 - kLpnFieldPos[j0], sh1 = 8 - kLpnFieldPos[j1];
      constexpr u32 m0 = ((1u << kLpnFieldBits[j0]) - 1) << 8, m1 = ((1u << kLpnFieldBits[j1]) - 1) << 8;
#define LPN_ADDR_PAIR(S0, S1, NOP)                                                                                             \
  asm(S0 " %0, %6, %4\n\t" S1 " %2, %7, %5\n\t" NOP                                                                       \
      "v_bitop3_b32 %0, %0, %8, %10 bitop3:0xea\n\tv_bitop3_b32 %2, %2, %9, %11 bitop3:0xea\n\t" NOP                      \
      "v_xor_b32 %1, 16, %0\n\tv_xor_b32 %3, 16, %2"                                                                        \
      : "=&v"(oa0), "=&v"(ob0), "=&v"(oa1), "=&v"(ob1)                                                                       \
      : "v"(dp[c0]), "v"(dp[c1]), "n"(sh0 >= 0 ? sh0 : -sh0), "n"(sh1 >= 0 ? sh1 : -sh1), "s"(m0), "s"(m1),                   \
        "v"(j0 == 4 ? xah[c0] : xa[c0]), "v"(j1 == 4 ? xah[c1] : xa[c1]))
#define LPN_ADDR_ONE(S, OA, OB, C, SH, M, J)                                                                                   \
  do {                                                                                                                         \
    u32 t_;                                                                                                                    \
    asm(S " %0, %1, %2" : "=v"(t_) : "n"(SH >= 0 ? SH : -SH), "v"(dp[C]));                                                     \
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xea" : "=v"(OA) : "v"(t_), "s"(M), "v"(J == 4 ? xah[C] : xa[C]));               \
    asm("v_xor_b32 %0, 16, %1" : "=v"(OB) : "v"(OA));                                                                          \
  } while (0)
      if constexpr ((ORD & 3) == 0) {  // separate statements (the compiler pads dependent pairs with s_nop and interleaves the reads)
        if constexpr (sh0 >= 0) LPN_ADDR_ONE("v_lshlrev_b32", oa0, ob0, c0, sh0, m0, j0);
        else LPN_ADDR_ONE("v_lshrrev_b32", oa0, ob0, c0, sh0, m0, j0);
        if constexpr (sh1 >= 0) LPN_ADDR_ONE("v_lshlrev_b32", oa1, ob1, c1, sh1, m1, j1);
        else LPN_ADDR_ONE("v_lshrrev_b32", oa1, ob1, c1, sh1, m1, j1);
      } else if constexpr ((ORD & 3) == 1) {
        if constexpr (sh0 >= 0 && sh1 >= 0) LPN_ADDR_PAIR("v_lshlrev_b32", "v_lshlrev_b32", "");
        else if constexpr (sh0 >= 0) LPN_ADDR_PAIR("v_lshlrev_b32", "v_lshrrev_b32", "");
        else if constexpr (sh1 >= 0) LPN_ADDR_PAIR("v_lshrrev_b32", "v_lshlrev_b32", "");
        else LPN_ADDR_PAIR("v_lshrrev_b32", "v_lshrrev_b32", "");
      } else {
        if constexpr (sh0 >= 0 && sh1 >= 0) LPN_ADDR_PAIR("v_lshlrev_b32", "v_lshlrev_b32", "s_nop 0\n\t");
        else if constexpr (sh0 >= 0) LPN_ADDR_PAIR("v_lshlrev_b32", "v_lshrrev_b32", "s_nop 0\n\t");
        else if constexpr (sh1 >= 0) LPN_ADDR_PAIR("v_lshrrev_b32", "v_lshlrev_b32", "s_nop 0\n\t");
        else LPN_ADDR_PAIR("v_lshrrev_b32", "v_lshrrev_b32", "s_nop 0\n\t");
      }
#undef LPN_ADDR_ONE
#undef LPN_ADDR_PAIR
      constexpr int imm0 = j0 == 4 ? kLpnGroupBase[4] - 65536 : kLpnGroupBase[j0];
      constexpr int imm1 = j1 == 4 ? kLpnGroupBase[4] - 65536 : kLpnGroupBase[j1];
      bl[st][0] = *reinterpret_cast<lds_cu32x4 *>(oa0 + (u32)imm0);
      bh[st][0] = *reinterpret_cast<lds_cu32x4 *>(ob0 + (u32)imm0);
      bl[st][1] = *reinterpret_cast<lds_cu32x4 *>(oa1 + (u32)imm1);
      bh[st][1] = *reinterpret_cast<lds_cu32x4 *>(ob1 + (u32)imm1);
    };
    auto fold = [&acc, &bl, &bh](auto ST) __attribute__((always_inline)) {
      constexpr int st = decltype(ST)::value;
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[0]) : "v"(bl[st][0].x), "v"(bl[st][1].x));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[1]) : "v"(bl[st][0].y), "v"(bl[st][1].y));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[2]) : "v"(bl[st][0].z), "v"(bl[st][1].z));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[3]) : "v"(bl[st][0].w), "v"(bl[st][1].w));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[4]) : "v"(bh[st][0].x), "v"(bh[st][1].x));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[5]) : "v"(bh[st][0].y), "v"(bh[st][1].y));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[6]) : "v"(bh[st][0].z), "v"(bh[st][1].z));
      asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[7]) : "v"(bh[st][0].w), "v"(bh[st][1].w));
    };
    if constexpr (ABL & 2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = dp[i];
    } else {
      issue(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
      issue(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
      static_for<20>([&](auto P) __attribute__((always_inline)) {
        constexpr int p = decltype(P)::value;
        if constexpr (p + 2 < 20) issue(std::integral_constant<int, p + 2>{}, std::integral_constant<int, (p + 2) % 3>{});
        __builtin_amdgcn_sched_barrier(0);
        fold(std::integral_constant<int, p % 3>{});
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    if (r < 8 && !(ABL & 8)) LPN_STAMP(5 + r, __builtin_amdgcn_s_memtime());
    // a lane with hsw set read the upper halves first: acc[0..3] are words 2, 3 of its row
    const long long wave_row = wave_row0 + (long long)r * step_rows;
    u32x4 f, g;
    f.x = acc[0], f.y = acc[1], f.z = acc[2], f.w = acc[3];
    g.x = acc[4], g.y = acc[5], g.z = acc[6], g.w = acc[7];
    if (MODE == 2 && wn == 4 && ldc == 4) {
      // wave-contiguous stores: after the swap f holds halves of rows 0..31 of the wave (lane j: half hsw of row j, lane j + 32 its
      // other half), g of rows 32..63
      lpn_swap32(f, g);
      u32x4 *c4 = reinterpret_cast<u32x4 *>(C) + wave_row * 2 + 2 * (lane & 31) + (hsw ^ (lane >> 5));
      if (wave_row + (lane & 31) < m) {
        if (accumulate) f ^= *c4;
        __builtin_nontemporal_store(f, c4);
      }
      if (wave_row + 32 + (lane & 31) < m) {
        if (accumulate) g ^= c4[64];
        __builtin_nontemporal_store(g, c4 + 64);
      }
    } else if (wave_row + lane < m) {
      u64 *dd = C + (wave_row + lane) * ldc;
      if (MODE >= 1 && wn == 4 && (ldc & 1) == 0) {
        u32x4 *d4 = reinterpret_cast<u32x4 *>(__builtin_assume_aligned(dd, 16));
        if (accumulate) f ^= d4[hsw], g ^= d4[hsw ^ 1];
        __builtin_nontemporal_store(f, d4 + hsw);
        __builtin_nontemporal_store(g, d4 + (hsw ^ 1));
      } else {
        u32 o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = lpn_pick(acc[i], acc[i ^ 4], 0u - (u32)hsw);
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if (w < wn) {
            u64 v = (u64)o[2 * w] | ((u64)o[2 * w + 1] << 32);
            if (accumulate) v ^= dd[w];
            dd[w] = v;
          }
      }
    }
  }
  LPN_STAMP(13, __builtin_amdgcn_s_memtime());
  LPN_STAMP(14, __builtin_amdgcn_s_memrealtime());
}
