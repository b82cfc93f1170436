// gf2_kernels_dev_thin.inc -- development-only kernels for products with few columns, with their launches: the retired tall-skinny
// kernels gf2_tallskinny4 / 5 / 6_kernel behind gf2k_dev_tallskinny (the hook of tallskinny_impl) and gf2k_tallskinny5_dbg, and the
// packed-B writer gf2_packB_kernel with gf2k_packB / gf2k_packB_chunks.  Not part of libm4ri_hip.so: included by
// m4ri-rust_amd/csrc/gf2_kernels.hip (above tallskinny_impl) only under -DGF2K_DEV_VARIANTS (tools/libm4ri_hip_dev.so; tools/kbench,
// tools/ts_stamps.py and the A/B switches M4RI_HIP_LPN, M4RI_HIP_TS6, M4RI_HIP_TALLSKINNY_OLD, M4RI_HIP_TS7 use them).  Needs what
// gf2_kernels.hip has at that point: u32 / u64, Log2, xor4, static_for, the lds_* typedefs, lds_limit_once, GF2K_DEV_ENV and the
// declaration of tallskinny3_launch.
//
// The round-2/3 kernels for l <= 256 (gf2_tallskinny5_kernel: 8-bit tables, two phases at n > 128; gf2_tallskinny6_kernel: 4-bit
// tables, small streaming workgroups) were replaced by gf2_lpn.inc in round 4 and no shape selects them any more: they are
// compiled into development builds only (tools/libm4ri_hip_dev.so, M4RI_HIP_LPN=0 for A/B runs).
// ---------------------------------------------------------------------------------------------
// tall-skinny kernel for an inner dimension of at most 256 bits (BASELINE config 5: l = 256) and 64 < n <= 256: the skewed
// lookups of gf2_tallskinny3_kernel with every row of A read exactly ONCE.
// gf2_tallskinny3_kernel fetches the words of a row again for every row set (16 bytes per lane and row: half of every
// 32-byte sector, once per row set -- 1.19x the algorithmic traffic at n = 256 and a load latency in the middle of the
// kernel each time).  Here a lane loads its RPT whole rows (32 bytes each, two 16-byte loads) before anything else, the 256
// rows of B are staged once, and the tables of 2 row sets (128 KiB: 256 bits of the inner dimension at NW = 2, 128 bits at
// NW = 4) are built per phase.  NW = 2 has ONE phase: a row goes through both row sets, is stored and forgotten (4 accumulator
// registers in all).  NW = 4 has two phases with 8 accumulator registers per row; it runs with 512 threads and 8 rows per
// lane so that 8 whole rows and their accumulators fit into registers.  The build of a phase needs only LDS, so the loads
// of A issued at the top stay in flight across it (the barriers wait for LDS operations only).
// ---------------------------------------------------------------------------------------------
template <int NW, int RPT, int NT, bool FULL, bool DBG = false, int EARLY = (RPT >= 8 ? 2 : 1), bool AHEAD = false>  // FULL: l in (192, 256], rows 16-byte aligned: two 16-byte loads per row, no branches
__global__ __launch_bounds__(NT) void gf2_tallskinny5_kernel(const u64 *__restrict__ A, long long lda, const u64 *__restrict__ B,
                                                              long long ldb, u64 *__restrict__ C, long long ldc, int m, int l,
                                                              int n, int accumulate, u64 *__restrict__ stamps = nullptr) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int TPR = 32 / NW;       // tables per row set (a 256-byte LDS row holds entry e of TPR tables)
  constexpr int ND = TPR / 4;        // dwords of a row that select inside one row set
  constexpr int WRS = TPR / 8;       // 64-bit words of the inner dimension per row set
  constexpr int SETS = NW == 1 ? 1 : 2;  // row sets in LDS at a time (64 KiB each); NW = 1: one row set holds all 256 bits
  constexpr int PHASES = 4 / (SETS * WRS);  // 4 words = SETS * WRS * PHASES
  const int tid = threadIdx.x, lane = tid & 63;
  const int wl = (l + 63) >> 6, wn = (n + 63) >> 6;
  const u64 maskL = (l & 63) ? ((1ull << (l & 63)) - 1) : ~0ull;
  const u64 maskC = (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;
  const long long row_base = (long long)blockIdx.x * (NT * RPT);
  const int s = lane & (TPR - 1);
  const u32 bsel = (s & 3) == 0 ? 0x03020100u : (s & 3) == 1 ? 0x02030001u : (s & 3) == 2 ? 0x01000302u : 0x00010203u;
  const int hsw = NW == 4 ? (lane >> 3) & 1 : 0;  // NW = 4: which 16-byte half this lane reads first
  const u32 xl0 = (u32)s * (8u * NW) + (u32)hsw * 16u, xl1 = xl0 + 65536u;
  auto lds_barrier = []() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  // DBG (development builds): wall-clock stamps (100 MHz) per wave: start, tables built, first row done, last row done
  u64 *st = nullptr;
  if constexpr (DBG) {
    st = stamps + ((long long)blockIdx.x * (NT / 64) + (tid >> 6)) * 8;
    if (lane == 0) st[0] = __builtin_amdgcn_s_memrealtime();
  }

  // ---- the 256 rows of B first (256 x NW words, one or two coalesced 8-byte loads per thread; rows past l are zero: their
  // tables select nothing): in-order return lets the build wait for them without waiting for the rows of A requested behind
  // them.  (Loading each build item's eight words of B straight from global memory instead -- scattered 8-byte loads, 128
  // instructions per CU ahead of the loads of A -- measured 0.9 us slower to the first table.)
  constexpr int ITEMS = SETS * TPR * NW * 16, IPT = (ITEMS + NT - 1) / NT;  // build items per phase, per thread
  constexpr int NB = (256 * NW + NT - 1) / NT;
  u64 bv[NB];
#pragma unroll
  for (int kk = 0; kk < NB; ++kk) {
    const int idx = tid + kk * NT, brow_ = idx / NW, w = idx % NW;
    bv[kk] = (idx < 256 * NW && brow_ < l && w < wn) ? B[(long long)brow_ * ldb + w] : 0;
  }
  // ---- every row of this lane, whole (words past the inner dimension read as zero).  Only the first row is requested
  // before the build: a CU holds a limited number of outstanding misses, and waves that cannot issue their loads would
  // reach the build barrier microseconds late (stamps: tables ready at 7.5 us with all rows requested up front) ----
  u64 aw[RPT][4];
  auto load_row = [&](int r) __attribute__((always_inline)) {
    const long long row = min(row_base + (long long)r * NT + tid, (long long)m - 1);  // clamped: stores are guarded
    const u64 *ap = A + row * lda;
    if constexpr (FULL) {  // straight-line code: the compiler can then wait for the rows one by one
      const uint4 *ap4 = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(ap, 16));
      const uint4 lo = ap4[0], hi = ap4[1];
      aw[r][0] = (u64)lo.x | ((u64)lo.y << 32);
      aw[r][1] = (u64)lo.z | ((u64)lo.w << 32);
      aw[r][2] = (u64)hi.x | ((u64)hi.y << 32);
      aw[r][3] = (u64)hi.z | ((u64)hi.w << 32);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) aw[r][q] = q < wl ? ap[q] : 0;
    }
  };
  // EARLY rows are requested before the first build; AHEAD: the others one row ahead of the lookups instead of all at once
#pragma unroll
  for (int r = 0; r < EARLY; ++r) load_row(r);
  u64 *bst = reinterpret_cast<u64 *>(lds + SETS * 65536);
#pragma unroll
  for (int kk = 0; kk < NB; ++kk)
    if (tid + kk * NT < 256 * NW) bst[tid + kk * NT] = bv[kk];
  lds_barrier();  // LDS operations only: the loads of A stay in flight across the build

  u32 acc[RPT][2 * NW];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
#pragma unroll
    for (int w = 0; w < 2 * NW; ++w) acc[r][w] = 0;

  auto store_row = [&](int r) {
    const long long row = row_base + (long long)r * NT + tid;
    if (row < m) {
      // NW = 4: lanes that read the upper half first hold words 2, 3 in acc[0..3] and words 0, 1 in acc[4..7]
      u32 o[2 * NW];
#pragma unroll
      for (int i = 0; i < 2 * NW; ++i) o[i] = (NW == 4 && hsw) ? acc[r][i ^ 4] : acc[r][i];
      if (FULL && NW >= 2 && wn == NW) {  // whole rows of C, 16 bytes per store (FULL also says: ldc even, C 16-byte aligned)
        const u32 mlo = (u32)maskC, mhi = (u32)(maskC >> 32);
        o[2 * NW - 2] &= mlo;
        o[2 * NW - 1] &= mhi;
        uint4 *dd = reinterpret_cast<uint4 *>(__builtin_assume_aligned(C + row * ldc, 16));
#pragma unroll
        for (int q = 0; q < NW / 2; ++q) {
          uint4 v = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
          if (accumulate) v = xor4(v, dd[q]);
          dd[q] = v;
        }
      } else {
#pragma unroll
        for (int w = 0; w < NW; ++w)
          if (w < wn) {
            u64 v = (u64)o[2 * w] | ((u64)o[2 * w + 1] << 32);
            if (w == wn - 1) v &= maskC;
            u64 *dd = C + row * ldc + w;
            if (accumulate) v ^= *dd;
            *dd = v;
          }
      }
    }
  };

#pragma unroll
  for (int ph = 0; ph < PHASES; ++ph) {
    if (ph * SETS * WRS * 64 >= l) break;  // uniform: nothing of the inner dimension left
    if (ph) lds_barrier();              // the previous phase's lookups are done
    // build: 4 select-XORs for the high nibble, 15 Gray-code steps for the 16 entries of the low nibble
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
      const int item = tid + it * NT;
      if (ITEMS % NT != 0 && item >= ITEMS) break;
      const int w = item % NW, t = (item / NW) % TPR;
      const int rest = item / (NW * TPR);
      const int rs = rest & (SETS - 1), h = rest / SETS;
      const u64 *rows = bst + (((ph * SETS + rs) * TPR + t) * 8) * NW + w;
      u64 v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) v ^= rows[(4 + b) * NW] & (0ull - (u64)((h >> b) & 1));
      const u64 r0 = rows[0], r1 = rows[NW], r2 = rows[2 * NW], r3 = rows[3 * NW];
      unsigned char *tb = lds + rs * 65536 + t * (8 * NW) + w * 8;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int gc = i ^ (i >> 1);
        if (i) {
          const int flip = __builtin_ctz(i);
          v ^= flip == 0 ? r0 : flip == 1 ? r1 : flip == 2 ? r2 : r3;
        }
        *reinterpret_cast<u64 *>(tb + (h * 16 + gc) * 256) = v;
      }
    }
    lds_barrier();
    if constexpr (DBG) {
      if (lane == 0) st[1 + 3 * ph] = __builtin_amdgcn_s_memrealtime();
    }
    if (ph == 0 && !AHEAD) {  // the remaining rows: nothing waits behind these requests but this wave's own lookups
#pragma unroll
      for (int r = EARLY; r < RPT; ++r) load_row(r);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      __builtin_amdgcn_sched_barrier(0);  // one row at a time
      if (AHEAD && ph == 0 && r + EARLY < RPT) load_row(r + EARLY);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rs = 0; rs < SETS; ++rs) {
        const int wi0 = (ph * SETS + rs) * WRS;
        if (wi0 * 64 < l) {  // uniform
          u32 d[ND];
#pragma unroll
          for (int q = 0; q < WRS; ++q) {
            u64 x = aw[r][wi0 + q];
            if (wi0 + q == wl - 1) x &= maskL;
            d[2 * q] = (u32)x;
            d[2 * q + 1] = (u32)(x >> 32);
          }
          // byte c of the permuted dwords = byte c ^ s of the row set's bytes
#pragma unroll
          for (int k = 0; (1 << k) < ND; ++k) {
            const bool sw = (s >> (2 + k)) & 1;
            u32 t2[ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) t2[i] = sw ? d[i ^ (1 << k)] : d[i];
#pragma unroll
            for (int i = 0; i < ND; ++i) d[i] = t2[i];
          }
#pragma unroll
          for (int i = 0; i < ND; ++i) d[i] = __builtin_amdgcn_perm(d[i], d[i], bsel);
          const u32 xl = rs ? xl1 : xl0;
#pragma unroll
          for (int c = 0; c < TPR; c += 2) {
            const u32 off = __builtin_amdgcn_perm(d[c >> 2], xl ^ (u32)(c * 8 * NW), 0x03020000u | ((4u + (c & 3)) << 8));
            const u32 off1 = __builtin_amdgcn_perm(d[(c + 1) >> 2], xl ^ (u32)((c + 1) * 8 * NW), 0x03020000u | ((4u + ((c + 1) & 3)) << 8));
            if constexpr (NW == 1) {
              const u32x2v v = *reinterpret_cast<lds_cu32x2 *>(off), w = *reinterpret_cast<lds_cu32x2 *>(off1);
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][0]) : "v"(v.x), "v"(w.x));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][1]) : "v"(v.y), "v"(w.y));
            } else {
              const u32x4 v = *reinterpret_cast<lds_cu32x4 *>(off), w = *reinterpret_cast<lds_cu32x4 *>(off1);
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][0]) : "v"(v.x), "v"(w.x));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][1]) : "v"(v.y), "v"(w.y));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][2]) : "v"(v.z), "v"(w.z));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][3]) : "v"(v.w), "v"(w.w));
            }
            if constexpr (NW == 4) {
              const u32x4 v2 = *reinterpret_cast<lds_cu32x4 *>(off ^ 16u), w2 = *reinterpret_cast<lds_cu32x4 *>(off1 ^ 16u);
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][4]) : "v"(v2.x), "v"(w2.x));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][5]) : "v"(v2.y), "v"(w2.y));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][6]) : "v"(v2.z), "v"(w2.z));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[r][7]) : "v"(v2.w), "v"(w2.w));
            }
          }
        }
      }
      // the last phase that holds bits of the inner dimension (uniform): the row is complete
      if ((ph + 1) * SETS * WRS * 64 >= l) store_row(r);
      if constexpr (DBG) {
        if ((r == 0 || r == RPT - 1) && lane == 0) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          st[2 + 3 * ph + (r ? 1 : 0)] = __builtin_amdgcn_s_memrealtime();
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// tall-skinny kernel with 4-BIT tables (n <= 256, l <= 256): small workgroups that stream.
// The kernels above build 8-bit tables (64 KiB per 256 bits of l at n = 64, up to 256 KiB at n = 256): one 512- or 1024-thread
// workgroup per CU, whose phases -- wait for B, build, wait for rows, look up, store -- every wave of the chip goes through at
// the same time, so that the HBM pipe idles during the build and the stores come in one burst.  With FOUR bits per table the
// tables of all 256 bits are 8 / 16 / 32 KiB for NW = 1 / 2 / 4 words per entry: a 256-thread workgroup builds them in a
// microsecond, eight (four) such workgroups fit a CU and run out of phase, and the rows stream through a grid-stride loop
// with the next row in flight -- the shape of gf2_narrow_kernel, which reaches the rate of a plain copy.  Twice the lookups
// (64 per row), but a 16-entry table spans each LDS bank at most once, so ANY mix of entries within a wave is conflict-free
// without skewing or byte permutations: lookup = shift, and, ds_read with the table's offset as an immediate.
// ---------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(256) void gf2_tallskinny6_kernel(const u64 *__restrict__ A, long long lda, const u64 *__restrict__ B,
                                                              long long ldb, u64 *__restrict__ C, long long ldc, int m, int l,
                                                              int n, int accumulate, int vec_ok) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int EB = 8 * NW;           // bytes per entry
  constexpr int TB = 16 * EB;          // bytes per table
  const int tid = threadIdx.x;
  const int wl = (l + 63) >> 6, wn = (n + 63) >> 6;
  const u64 maskL = (l & 63) ? ((1ull << (l & 63)) - 1) : ~0ull;
  const u64 maskC = (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + tid;
  u64 *bst = reinterpret_cast<u64 *>(lds + 64 * TB);  // the 256 rows of B, NW words each

  // B first (in-order return: the build then does not wait for the row requested behind it), then this lane's first row
  u64 bv[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) bv[w] = (tid < l && w < wn) ? B[(long long)tid * ldb + w] : 0;
  u64 cur[4];
  auto load_row = [&](long long row, u64 (&a)[4]) __attribute__((always_inline)) {
    const u64 *ar = A + row * lda;
    if (vec_ok) {  // l > 192, 16-byte aligned rows: two 16-byte loads
      const uint4 lo = *reinterpret_cast<const uint4 *>(ar), hi = *reinterpret_cast<const uint4 *>(ar + 2);
      a[0] = (u64)lo.x | ((u64)lo.y << 32);
      a[1] = (u64)lo.z | ((u64)lo.w << 32);
      a[2] = (u64)hi.x | ((u64)hi.y << 32);
      a[3] = (u64)hi.z | ((u64)hi.w << 32);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = q < wl ? ar[q] : 0;
    }
  };
  if (i < m) load_row(i, cur);
#pragma unroll
  for (int w = 0; w < NW; ++w) bst[tid * NW + w] = bv[w];
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only
  __builtin_amdgcn_s_barrier();
  // build: 64 tables x 16 entries; entry e of table t = XOR of rows 4t + b of B for the set bits b of e
  for (int idx = tid; idx < 64 * 16; idx += 256) {
    const int t = idx >> 4, e = idx & 15;
    u64 v[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) v[w] = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const u64 sel = 0ull - (u64)((e >> b) & 1);
#pragma unroll
      for (int w = 0; w < NW; ++w) v[w] ^= bst[(4 * t + b) * NW + w] & sel;
    }
    u64 *dst = reinterpret_cast<u64 *>(lds + idx * EB);
#pragma unroll
    for (int w = 0; w < NW; ++w) dst[w] = v[w];
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();

  for (; i < m; i += stride) {
    u32 d[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u64 x = (q == wl - 1) ? (cur[q] & maskL) : cur[q];
      d[2 * q] = (u32)x;
      d[2 * q + 1] = (u32)(x >> 32);
    }
    if (i + stride < m) load_row(i + stride, cur);  // the next row of this lane: in flight during the lookups
    u32 acc[2 * NW];
#pragma unroll
    for (int w = 0; w < 2 * NW; ++w) acc[w] = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      // the eight entry offsets of a dword, pre-scaled, as the bytes of two registers (even nibbles in xe, odd ones in xo): one
      // byte extraction per lookup instead of a shift and a mask
      u32 xe = (d[q] & 0x0f0f0f0fu) * (u32)EB, xo = ((d[q] >> 4) & 0x0f0f0f0fu) * (u32)EB;
      asm("" : "+v"(xe), "+v"(xo));  // (opaque: the optimiser would fold the bytes back into eight shift-and-mask pairs)
#pragma unroll
      for (int k = 0; k < 8; k += 2) {  // nibbles k and k + 1 of dword q: tables 8 q + k, 8 q + k + 1 (offsets fold to immediates)
        const u32 t0 = (u32)(8 * q + k) * TB, t1 = t0 + TB;
        const u32 o0 = EB <= 16 ? __builtin_amdgcn_ubfe(xe, 4 * k, 8) : ((d[q] >> (4 * k)) & 15u) * EB,
                  o1 = EB <= 16 ? __builtin_amdgcn_ubfe(xo, 4 * k, 8) : ((d[q] >> (4 * k + 4)) & 15u) * EB;
        if constexpr (NW == 1) {
          const u32x2v x = *reinterpret_cast<lds_cu32x2 *>(o0 + t0), y = *reinterpret_cast<lds_cu32x2 *>(o1 + t1);
          asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[0]) : "v"(x.x), "v"(y.x));
          asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[1]) : "v"(x.y), "v"(y.y));
        } else {
          const u32x4 x = *reinterpret_cast<lds_cu32x4 *>(o0 + t0), y = *reinterpret_cast<lds_cu32x4 *>(o1 + t1);
          asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[0]) : "v"(x.x), "v"(y.x));
          asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[1]) : "v"(x.y), "v"(y.y));
          asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[2]) : "v"(x.z), "v"(y.z));
          asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[3]) : "v"(x.w), "v"(y.w));
          if constexpr (NW == 4) {
            const u32x4 x2 = *reinterpret_cast<lds_cu32x4 *>(o0 + t0 + 16u), y2 = *reinterpret_cast<lds_cu32x4 *>(o1 + t1 + 16u);
            asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[4]) : "v"(x2.x), "v"(y2.x));
            asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[5]) : "v"(x2.y), "v"(y2.y));
            asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[6]) : "v"(x2.z), "v"(y2.z));
            asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(acc[7]) : "v"(x2.w), "v"(y2.w));
          }
        }
      }
    }
    u64 *dd = C + i * ldc;
#pragma unroll
    for (int w = 0; w < NW; ++w)
      if (w < wn) {
        u64 v = (u64)acc[2 * w] | ((u64)acc[2 * w + 1] << 32);
        if (w == wn - 1) v &= maskC;
        if (accumulate) v ^= dd[w];
        dd[w] = v;
      }
  }
}

// tall-skinny kernel with conflict-free lookups and no byte permutation ("generation" kernel; n <= 256).
// The first kernel's lookups collide in the LDS banks (8-byte entries: 32 lanes on 32 random bank pairs, ~3.5 lanes on the
// busiest); the skewed kernel avoids that by spreading the lanes over 32 / NW tables, which costs a byte permutation of every
// row and reloads A after every table build.  Here the skew stays inside one 64-bit word of the row -- lane L visits its 8
// chunks in the order c ^ (L & 7), and the selecting byte comes out of the two dwords of the word with ONE v_perm_b32 whose
// selector is per lane -- and whatever is missing to fill a 256-byte LDS row comes from COPIES of every table: the row holds
// entry e of 8 chunks x (4 / NW) copies x 8 NW bytes (slot = copies * chunk + copy), so the lanes the LDS serves together
// read different slots whatever their entries are (NW = 4: one copy, the two 16-byte halves of an entry are read in opposite
// order by lanes 8..15 of every 16, as in the skewed kernel).
// A "generation" = the tables of one 64-bit word of the inner dimension = 64 KiB; two generations are resident (one being
// looked up while the next is built, ONE barrier per generation, and that barrier waits for LDS operations only, so the loads
// of A issued at the top stay in flight across the builds); rows of the table are written with one ds_write_addtid_b32 each
// (lane = dword of the row), Gray-code order, like the tile kernels; the rows of B of four generations are staged in LDS.
// One lane per row of A, RPT rows per lane, two chunks per three-input XOR.
// ---------------------------------------------------------------------------------------------
template <int NW, int RPT, int NT>
__global__ __launch_bounds__(NT) void gf2_tallskinny4_kernel(const u64 *__restrict__ A, long long lda, const u64 *__restrict__ B,
                                                              long long ldb, u64 *__restrict__ C, long long ldc, int m, int l,
                                                              int n, int accumulate) {
  extern __shared__ __align__(16) unsigned char lds[];
  constexpr int WAVES = NT / 64, EPW = 256 / WAVES, LOWB = Log2<EPW>::value;
  constexpr int COPIES = 4 / NW, EB = 8 * NW;  // copies of a table in an LDS row, bytes per entry
  static_assert(EPW * WAVES == 256 && EPW >= 1 && (NW == 1 || NW == 2 || NW == 4), "geometry");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wl = (l + 63) >> 6, wn = (n + 63) >> 6;
  const u64 maskL = (l & 63) ? ((1ull << (l & 63)) - 1) : ~0ull;
  const u64 maskC = (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;
  const long long row_base = (long long)blockIdx.x * (NT * RPT);
  // lookups: chunk order c ^ s, copy cp; NW = 4: lanes with hsw read the upper 16 bytes of an entry first
  const int s = lane & 7, cp = (lane >> 3) & (COPIES - 1);
  const int hsw = NW == 4 ? (lane >> 3) & 1 : 0;
  u32 selc[8], loc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int cs = c ^ s;
    selc[c] = 0x0c0c000cu | ((u32)cs << 8);  // {0, 0, byte cs of the 64-bit word, 0}: v_perm_b32(high dword, low dword, sel)
    loc[c] = (u32)((cs * COPIES + cp) * EB + hsw * 16);
  }
  // build: lane = dword of the 256-byte table row: slot = lane / (2 NW) = COPIES * chunk + copy, dword lane % (2 NW) of the entry
  const int bch = (lane / (2 * NW)) / COPIES, bdw = lane % (2 * NW);

  u32 acc[RPT][2 * NW];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
#pragma unroll
    for (int w = 0; w < 2 * NW; ++w) acc[r][w] = 0;

  // barrier that waits for this wave's LDS operations only: the loads of A stay in flight across it
  auto lds_barrier = []() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  u64 *bstage = reinterpret_cast<u64 *>(lds + 128 * 1024);  // the 256 rows of B of a block of four generations (2 NW KiB)

  for (int w0 = 0; w0 < wl; w0 += 4) {  // four 64-bit words of the inner dimension = four generations
    // the block's rows of B first (one or two coalesced loads per thread): in-order return then lets the staging wait for
    // them without waiting for the rows of A requested behind them
    constexpr int NBV = (256 * NW + NT - 1) / NT;
    u64 bvals[NBV];
#pragma unroll
    for (int kk = 0; kk < NBV; ++kk) {
      const int idx = tid + kk * NT;
      const long long brow = (long long)w0 * 64 + idx / NW;
      const int w = idx % NW;
      bvals[kk] = (idx < 256 * NW && brow < l && w < wn) ? B[brow * ldb + w] : 0;
    }
    // HALF of this lane's rows are requested before the barriers, the other half behind them: a CU holds a limited number
    // of outstanding misses, and with all RPT rows requested up front the waves that could not issue their loads reached
    // the staging barrier microseconds late (per-wave stamps: first table at 7.5 us instead of 3)
    u64 aw[RPT][4];
    auto load_row = [&](int r) __attribute__((always_inline)) {
      const long long row = min(row_base + (long long)r * NT + tid, (long long)m - 1);  // clamped: stores are guarded
      const u64 *ap = A + row * lda;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        u64 x = ap[min(w0 + q, wl - 1)];
        if (w0 + q >= wl) x = 0;
        if (w0 + q == wl - 1) x &= maskL;
        aw[r][q] = x;
      }
    };
    constexpr int EARLY4 = RPT > 1 ? RPT / 2 : 1;
#pragma unroll
    for (int r = 0; r < EARLY4; ++r) load_row(r);
    lds_barrier();  // every wave is done with the previous block's rows of B
#pragma unroll
    for (int kk = 0; kk < NBV; ++kk)
      if (tid + kk * NT < 256 * NW) bstage[tid + kk * NT] = bvals[kk];
    lds_barrier();
#pragma unroll
    for (int r = EARLY4; r < RPT; ++r) load_row(r);
    static_for<4>([&](auto gtag) __attribute__((always_inline)) {
      constexpr int g = decltype(gtag)::value;
      constexpr u32 tbase = (g & 1) ? 65536u : 0u;  // w0 is a multiple of 4: generation w0 + g lives in buffer g & 1
      if (w0 + g < wl) {                            // uniform
        // ---- build the generation: wave w owns entries [EPW w, EPW (w + 1)) ----
        u32 rr[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) rr[b] = reinterpret_cast<const u32 *>(bstage + (g * 64 + bch * 8 + b) * NW)[bdw];
        u32 cur = 0;
#pragma unroll
        for (int b = LOWB; b < 8; ++b)
          if ((wave >> (b - LOWB)) & 1) cur ^= rr[b];
        {
          constexpr u32 kOff = tbase ? (0x10004u - (u32)(EPW * 256)) : 0u;  // see gf2_m4rm_kernel_v3
          const u32 m0v = tbase + (u32)wave * (u32)(EPW * 256) - kOff;
          asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(m0v) : "memory");  // (one wait state before an LDS add-TID instruction reads M0: the compiler cannot see that the asm below does)
          static_for<EPW>([&](auto itag) __attribute__((always_inline)) {
            constexpr int i = decltype(itag)::value;
            constexpr unsigned e = (unsigned)i ^ ((unsigned)i >> 1);
            if constexpr (i > 0) cur ^= rr[__builtin_ctz(i | 256)];
            asm volatile("ds_write_addtid_b32 %0 offset:%1" ::"v"(cur), "n"(kOff + e * 256u) : "memory");
          });
        }
        lds_barrier();  // the generation is complete; every wave has also finished the lookups of generation - 2 in this buffer
        // ---- lookups ----
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const u32 a0 = (u32)aw[r][g], a1 = (u32)(aw[r][g] >> 32);
          u32 ac[2 * NW];  // (locals: an asm operand inside this lambda cannot name the enclosing function's array)
#pragma unroll
          for (int w = 0; w < 2 * NW; ++w) ac[w] = acc[r][w];
#pragma unroll
          for (int c = 0; c < 8; c += 2) {
            const u32 o0 = __builtin_amdgcn_perm(a1, a0, selc[c]) | loc[c];
            const u32 o1 = __builtin_amdgcn_perm(a1, a0, selc[c + 1]) | loc[c + 1];
            if constexpr (NW == 1) {
              const u32x2v x = *reinterpret_cast<lds_cu32x2 *>(o0), y = *reinterpret_cast<lds_cu32x2 *>(o1);
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[0]) : "v"(x.x), "v"(y.x));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[1]) : "v"(x.y), "v"(y.y));
            } else {
              const u32x4 x = *reinterpret_cast<lds_cu32x4 *>(o0), y = *reinterpret_cast<lds_cu32x4 *>(o1);
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[0]) : "v"(x.x), "v"(y.x));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[1]) : "v"(x.y), "v"(y.y));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[2]) : "v"(x.z), "v"(y.z));
              asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[3]) : "v"(x.w), "v"(y.w));
              if constexpr (NW == 4) {
                const u32x4 x2 = *reinterpret_cast<lds_cu32x4 *>(o0 ^ 16u), y2 = *reinterpret_cast<lds_cu32x4 *>(o1 ^ 16u);
                asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[4]) : "v"(x2.x), "v"(y2.x));
                asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[5]) : "v"(x2.y), "v"(y2.y));
                asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[6]) : "v"(x2.z), "v"(y2.z));
                asm("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(ac[7]) : "v"(x2.w), "v"(y2.w));
              }
            }
          }
#pragma unroll
          for (int w = 0; w < 2 * NW; ++w) acc[r][w] = ac[w];
        }
      }
      // the next generation lives in the other buffer
#pragma unroll
      for (int c = 0; c < 8; ++c) loc[c] ^= 65536u;
    });
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const long long row = row_base + (long long)r * NT + tid;
    if (row < m) {
#pragma unroll
      for (int w = 0; w < NW; ++w)
        if (w < wn) {
          // NW = 4: lanes that read the upper half first hold words 2, 3 in acc[0..3] and words 0, 1 in acc[4..7]
          u32 lo = acc[r][2 * w], hi = acc[r][2 * w + 1];
          if constexpr (NW == 4) {
            lo = hsw ? acc[r][(2 * w) ^ 4] : lo;
            hi = hsw ? acc[r][(2 * w + 1) ^ 4] : hi;
          }
          u64 v = (u64)lo | ((u64)hi << 32);
          if (w == wn - 1) v &= maskC;
          u64 *d = C + row * ldc + w;
          if (accumulate) v ^= *d;
          *d = v;
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// B (l x n, row-major) -> chunk-packed layout of the tile kernel (see gf2_m4rm_kernel_v3, BPACK).
// thread <-> (chunk c, column tile tn, lane d): reads dword d of rows 8c..8c+7 (a wave reads 256 contiguous bytes of
// each row), writes its 32 bytes (a wave writes one whole 2 KiB block).  Rows >= l, columns >= n and the nc - ceil(l/8)
// padding chunks are written as zeros.  blockIdx.z = batch.
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void gf2_packB_kernel(u32 *__restrict__ Bp, long long bpStride, const u64 *__restrict__ B,
                                                        long long ldb, long long bStride, int l, int n, int nc, int tiles_n) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int tn = blockIdx.y;
  if (c >= nc) return;
  const u32 *B32 = reinterpret_cast<const u32 *>(B + (long long)blockIdx.z * bStride);
  const int ndw = ((n + 63) >> 6) * 2;  // dwords per row that exist
  const int dcol = tn * 64 + lane;
  const u32 tail = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xffffffffu;
  u32 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int row = c * 8 + r;
    u32 x = 0;
    if (row < l && dcol < ndw) {
      x = B32[(long long)row * ldb * 2 + dcol];
      if (dcol == ((n + 31) >> 5) - 1) x &= tail;
      if (dcol > ((n + 31) >> 5) - 1) x = 0;
    }
    v[r] = x;
  }
  uint4 *dst = reinterpret_cast<uint4 *>(Bp + ((long long)blockIdx.z * bpStride + ((long long)tn * nc + c) * 512) + lane * 8);
  dst[0] = make_uint4(v[0], v[1], v[2], v[3]);
  dst[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// chunks per tile column of a packed operand with inner dimension l (4 padding chunks: the kernel prefetches two
// chunks past the last 32-bit word)
extern "C" int gf2k_packB_chunks(int l) { return ((l + 31) / 32) * 4 + 4; }

// bpStride: dwords between batch elements of Bp (>= tiles_n * gf2k_packB_chunks(l) * 512)
extern "C" hipError_t gf2k_packB(uint32_t *Bp, long long bpStride, const u64 *B, long long ldb, long long bStride, int l,
                                 int n, int batch, hipStream_t stream) {
  if (l <= 0 || n <= 0 || batch <= 0) return hipSuccess;
  const int nc = gf2k_packB_chunks(l), tiles_n = (n + 2047) / 2048;
  hipLaunchKernelGGL(gf2_packB_kernel, dim3((nc + 3) / 4, tiles_n, batch), dim3(256), 0, stream, Bp, bpStride, B, ldb,
                     bStride, l, n, nc, tiles_n);
  return hipGetLastError();
}

// The hook of tallskinny_impl (gf2_kernels.hip), called after its argument checks with the same arguments: *took = false when no switch
// is set for this product (the shipped dispatch goes on), otherwise the product has been launched here and the result is the call's.
// Which kernel took a tall-skinny product before round 4, and takes it again under the switches (n <= 256; measured cold at
// 2^20 x 256, us):
//   l <= 256, n <= 64        gf2_tallskinny6_kernel<1>   4-bit tables, small streaming workgroups       11.8  (generation kernel 15.0)
//   l <= 256, 64 < n <= 128  gf2_tallskinny5_kernel<2>   8-bit tables, whole rows read once, one phase  14.7  (4-bit form 16.0)
//   l <= 256, 128 < n        gf2_tallskinny5_kernel<4>   the same in two phases, 512 threads x 8 rows   20.9  (4-bit form 35.7)
//   256 < l, n <= 64         gf2_tallskinny4_kernel<1>   generations of 64 bits of l, one built while the previous is looked up
//   256 < l, 64 < n          gf2_tallskinny3_kernel<NW>  row sets of 32 / NW tables, rows re-fetched per row set (shipped)
// M4RI_HIP_LPN=0 restores the first three rows (the round-2/3 kernels); M4RI_HIP_TS6 = mask of the entry widths (1, 2, 4 words) the
// 4-bit kernel takes instead (default 1); M4RI_HIP_TALLSKINNY_OLD=1 sends l <= 256 to the round-1 kernels (the last two rows); the
// fourth row is reached by callers that keep such shapes from gf2k_tallskinny_long (M4RI_HIP_TS7=0).  None of them packs `side`.
static hipError_t gf2k_dev_tallskinny(const u64 *A, long long lda, const u64 *B, long long ldb, u64 *C, long long ldc, int m, int l, int n,
                                      int accumulate, u64 *side, long long side_ld, hipStream_t stream, bool *took) {
  const int nw = (n + 63) / 64;
  static const int old_only = GF2K_DEV_ENV("M4RI_HIP_TALLSKINNY_OLD", 0);
  static const int ts6 = GF2K_DEV_ENV("M4RI_HIP_TS6", 1);
  static const int lpn = GF2K_DEV_ENV("M4RI_HIP_LPN", 1);
  *took = !(l <= 256 && !old_only && lpn) && (side || l <= 256 || nw == 1);
  if (!*took) return hipSuccess;  // gf2_lpn.inc, or 256 < l with more than one word of C: the shipped launches
  if (side) return hipErrorNotSupported;
  if (l <= 256 && !old_only && (ts6 & (nw == 3 ? 4 : nw))) {
    const int vec_ok = l > 192 && (lda & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
    long long blocks = ((long long)m + 255) / 256;
    static const int cap_env = GF2K_DEV_ENV("M4RI_HIP_TS6_BLOCKS", 0);  // (A/B measurements)
    const long long cap = cap_env > 0 ? cap_env : (nw <= 2 ? 2048 : 1024);  // 8 (4) workgroups per CU
    if (blocks > cap) blocks = cap;
#define GF2_TS6_LAUNCH(NWV)                                                                                                       \
  do {                                                                                                                            \
    const size_t lds6 = 64 * 16 * 8 * NWV + 256 * 8 * NWV;                                                                        \
    hipLaunchKernelGGL((gf2_tallskinny6_kernel<NWV>), dim3((unsigned)blocks), dim3(256), lds6, stream, A, lda, B, ldb, C, ldc, m, l, n, \
                       accumulate, vec_ok);                                                                                       \
  } while (0)
    if (nw == 1) GF2_TS6_LAUNCH(1);
    else if (nw == 2) GF2_TS6_LAUNCH(2);
    else GF2_TS6_LAUNCH(4);
#undef GF2_TS6_LAUNCH
    return hipGetLastError();
  }
  if (nw >= 2 && l <= 256 && !old_only) {  // every row of A read once (gf2_tallskinny5_kernel)
    const size_t lds5 = 128 * 1024 + 256 * 8 * (nw <= 2 ? 2 : 4);
    const bool full = l > 192 && ((lda | ldc) & 1) == 0 && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(C)) & 15) == 0;
    hipError_t e5 = hipSuccess;
#define GF2_TS5_LAUNCH(NWV, RPTV, NTV, FULLV, EV)                                                                             \
  do {                                                                                                                      \
    e5 = lds_limit_once(reinterpret_cast<const void *>(&gf2_tallskinny5_kernel<NWV, RPTV, NTV, FULLV, false, EV, true>), (int)lds5); \
    if (e5 != hipSuccess) return e5;                                                                                        \
    const unsigned grid5 = (unsigned)(((long long)m + NTV * RPTV - 1) / (NTV * RPTV));                                      \
    hipLaunchKernelGGL((gf2_tallskinny5_kernel<NWV, RPTV, NTV, FULLV, false, EV, true>), dim3(grid5), dim3(NTV), lds5, stream, A, lda, B, ldb, C, \
                       ldc, m, l, n, accumulate);                                                                           \
  } while (0)
    // rows requested before the first build (EARLY) / the others one row ahead of the lookups: per-wave stamps, cold A
    if (nw == 2 && full) GF2_TS5_LAUNCH(2, 4, 1024, true, 1);
    else if (nw == 2) GF2_TS5_LAUNCH(2, 4, 1024, false, 1);
    else if (full) GF2_TS5_LAUNCH(4, 8, 512, true, 2);
    else GF2_TS5_LAUNCH(4, 8, 512, false, 2);
#undef GF2_TS5_LAUNCH
    return hipGetLastError();
  }
  if (nw == 1) {  // generation kernel (replicated tables, skew inside a 64-bit word)
    constexpr int RPT4 = 4, NT4 = 1024;
    const unsigned grid4 = (unsigned)(((long long)m + NT4 * RPT4 - 1) / (NT4 * RPT4));
    const size_t lds4 = 128 * 1024 + 8 * 1024;
    hipError_t e4 = lds_limit_once(reinterpret_cast<const void *>(&gf2_tallskinny4_kernel<1, RPT4, NT4>), (int)lds4);
    if (e4 != hipSuccess) return e4;
    hipLaunchKernelGGL((gf2_tallskinny4_kernel<1, RPT4, NT4>), dim3(grid4), dim3(NT4), lds4, stream, A, lda, B, ldb, C, ldc, m, l, n,
                       accumulate);
    return hipGetLastError();
  }
  return tallskinny3_launch(A, lda, B, ldb, C, ldc, m, l, n, accumulate, stream);  // M4RI_HIP_TALLSKINNY_OLD=1, more than one word of C
}

// development: gf2_tallskinny5_kernel with wall-clock stamps (8 u64 per wave: start, then per phase: built, first row, last row)
extern "C" hipError_t gf2k_tallskinny5_dbg(const u64 *A, long long lda, const u64 *B, long long ldb, u64 *C, long long ldc, int m,
                                           int l, int n, u64 *stamps, hipStream_t stream) {
  const int nw = (n + 63) / 64;
  const size_t lds5 = (nw == 1 ? 64 : 128) * 1024 + 256 * 8 * nw;
  const int variant = getenv("TS5_VARIANT") ? atoi(getenv("TS5_VARIANT")) : 0;  // 10 * EARLY + AHEAD
#define TS5_DBG(NWV, RPTV, NTV, EARLYV, AHEADV)                                                                                   \
  do {                                                                                                                            \
    hipError_t e = lds_limit_once(reinterpret_cast<const void *>(&gf2_tallskinny5_kernel<NWV, RPTV, NTV, true, true, EARLYV, AHEADV>), \
                                  (int)lds5);                                                                                     \
    if (e != hipSuccess) return e;                                                                                                \
    hipLaunchKernelGGL((gf2_tallskinny5_kernel<NWV, RPTV, NTV, true, true, EARLYV, AHEADV>), dim3((m + NTV * RPTV - 1) / (NTV * RPTV)), \
                       dim3(NTV), lds5, stream, A, lda, B, ldb, C, ldc, m, l, n, 0, stamps);                                      \
  } while (0)
  if (nw == 1) {
    switch (variant) {
      case 111: TS5_DBG(1, 8, 512, 1, true); break;
      case 121: TS5_DBG(1, 8, 512, 2, true); break;
      case 211: TS5_DBG(1, 4, 512, 1, true); break;
      case 221: TS5_DBG(1, 4, 512, 2, true); break;
      case 240: TS5_DBG(1, 4, 512, 4, false); break;
      case 311: TS5_DBG(1, 2, 512, 1, true); break;
      case 320: TS5_DBG(1, 2, 512, 2, false); break;
      default: TS5_DBG(1, 4, 1024, 1, true); break;
    }
  } else if (nw == 2) {
    switch (variant) {
      case 10: TS5_DBG(2, 4, 1024, 1, false); break;
      case 11: TS5_DBG(2, 4, 1024, 1, true); break;
      case 20: TS5_DBG(2, 4, 1024, 2, false); break;
      case 21: TS5_DBG(2, 4, 1024, 2, true); break;
      case 31: TS5_DBG(2, 4, 1024, 3, true); break;
      case 111: TS5_DBG(2, 8, 512, 1, true); break;
      case 121: TS5_DBG(2, 8, 512, 2, true); break;
      case 131: TS5_DBG(2, 8, 512, 3, true); break;
      case 141: TS5_DBG(2, 8, 512, 4, true); break;
      default: TS5_DBG(2, 4, 1024, 1, false); break;
    }
  } else {
    switch (variant) {
      case 10: TS5_DBG(4, 8, 512, 1, false); break;
      case 11: TS5_DBG(4, 8, 512, 1, true); break;
      case 21: TS5_DBG(4, 8, 512, 2, true); break;
      case 31: TS5_DBG(4, 8, 512, 3, true); break;
      case 41: TS5_DBG(4, 8, 512, 4, true); break;
      default: TS5_DBG(4, 8, 512, 2, false); break;
    }
  }
#undef TS5_DBG
  return hipGetLastError();
}
