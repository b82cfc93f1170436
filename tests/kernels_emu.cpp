// kernels_emu.cpp -- runs the word-level kernels of m4ri-rust_amd/csrc thread by thread on the CPU (tests/test_kernels_cpu.py cuts
// their shipped text out of the .hip files with tests/kernel_text.py into KERNEL_BODY and builds this file with the host compiler and
// its address / undefined-behaviour sanitizers; the stand-ins for the HIP names are tests/kernel_emu.h).  Three programs come out of
// it, compiled and run side by side: -DEMU_STREAM (the streaming helpers of gf2_kernels.hip), -DEMU_STRASSEN (its level passes, which
// alone take the compiler most of the time) and -DEMU_REST (gf2_ple.hip, gf2_trsm.hip, gf2_nullspace.hip, gf2_elim.hip).
//
// Rules every driver below follows (those of blocks_emu.cpp):
//   * every buffer is an exact malloc of (rows - 1) * ld + width words: the red zone starts right behind the last word of the last
//     row, so a load or store of a word that holds no bit of the operand is a report;
//   * bases are 16-byte aligned and 8 bytes off, ld runs over width, width + 1, width + 2 -- except where the host code that calls
//     the launcher rules a combination out; the precondition is then quoted beside the driver;
//   * content is random, the expectation is computed with plain loops written here (never by calling library code), and the WHOLE
//     destination buffer is compared, so a changed bit outside the region fails;
//   * where a launcher exists in the kernel file it is the launcher that is called: its `vec` decision and its launch shape are then
//     what the alignment check judges.
// What this cannot show: ordering between threads, cross-lane semantics, performance.
#include "kernel_emu.h"
#include "gf2_variants.h"  // plain C++: the Strassen table's initialiser that the split3 kernel names
#define GF2K_DEV_ENV(name, dflt) (dflt)
#include KERNEL_BODY

static std::mt19937_64 rng(20240607);

#define FAIL(...)                  \
  do {                             \
    printf("MISMATCH " __VA_ARGS__); \
    printf("\n");                  \
    exit(1);                       \
  } while (0)

// an exact allocation of n elements, `off` elements behind a 16-byte boundary, random content
template <typename T>
struct Exact {
  char *raw;
  T *p;
  long long n;
  Exact(long long n_, int off_bytes = 0) : n(n_) {
    raw = (char *)malloc((size_t)n_ * sizeof(T) + off_bytes);
    if ((uintptr_t)raw & 15) { printf("malloc not 16-aligned\n"); exit(2); }
    p = (T *)(raw + off_bytes);
    unsigned char *b = (unsigned char *)p;
    for (size_t i = 0; i < (size_t)n_ * sizeof(T); ++i) b[i] = (unsigned char)rng();
  }
  Exact(const Exact &) = delete;
  ~Exact() { free(raw); }
  std::vector<T> snap() const { return std::vector<T>(p, p + n); }
  T &operator[](long long i) { return p[i]; }
};
typedef Exact<u64> Words;
static long long span(long long rows, long long ld, long long width) { return rows <= 0 ? 0 : (rows - 1) * ld + width; }
static int wordsof(long long bits) { return (int)((bits + 63) / 64); }
static u64 lastmask(long long bits) { return (bits & 63) ? ((1ull << (bits & 63)) - 1) : ~0ull; }
static int getbit(const u64 *row, long long c) { return (int)((row[c >> 6] >> (c & 63)) & 1); }
static void check(const Words &got, const std::vector<u64> &want, const char *what, long long a = 0, long long b = 0, long long c = 0,
                  long long d = 0) {
  for (long long i = 0; i < got.n; ++i)
    if (got.p[i] != want[i]) FAIL("%s (%lld %lld %lld %lld): word %lld is %016llx, want %016llx", what, a, b, c, d, i,
                                  (unsigned long long)got.p[i], (unsigned long long)want[i]);
}
static const int kRowsNarrow[] = {1, 2, 3, 4, 5, 300};  // 300 only for rows of up to three words
static const int kCols[] = {1, 63, 64, 65, 127, 128, 129, 200};

#ifdef EMU_STREAM
// ---------------------------------------------------------------------------------------------------------------------------------
// gf2_kernels.hip
// ---------------------------------------------------------------------------------------------------------------------------------

// gf2k_xor2d: C = A ^ B, copy (B null, ld 0), zero (both null), in place (C is A; C is B).  Every ld and base of every operand.
static long run_xor2d() {
  long cases = 0;
  for (int words = 1; words <= 4; ++words)
    for (int rows : kRowsNarrow) {
      if (rows == 300 && words > 3) continue;
      for (int mode = 0; mode < 5; ++mode)  // 0: A, B; 1: A alone; 2: neither; 3: C is A; 4: C is B
        for (int g = 0; g < 27 * 8; ++g) {
          const int dc = g % 3, da = g / 3 % 3, db = g / 9 % 3, oc = g / 27 & 1, oa = g / 54 & 1, ob = g / 108 & 1;
          if ((mode == 1 || mode == 2) && (db || ob)) continue;  // no B: nothing to vary
          if (mode == 2 && (da || oa)) continue;
          if (mode == 3 && (da || oa)) continue;  // A follows C
          if (mode == 4 && (db || ob)) continue;
          const long long ldc = words + dc, lda = words + da, ldb = words + db;
          Words C(span(rows, ldc, words), 8 * oc), A(span(rows, lda, words), 8 * oa), B(span(rows, ldb, words), 8 * ob);
          const u64 *a = mode == 2 ? nullptr : mode == 3 ? C.p : A.p, *b = mode == 1 || mode == 2 ? nullptr : mode == 4 ? C.p : B.p;
          const long long la = mode == 2 ? 0 : mode == 3 ? ldc : lda, lb = mode == 1 || mode == 2 ? 0 : mode == 4 ? ldc : ldb;
          std::vector<u64> want = C.snap();
          for (int r = 0; r < rows; ++r)
            for (int w = 0; w < words; ++w) want[r * ldc + w] = (a ? a[r * la + w] : 0) ^ (b ? b[r * lb + w] : 0);
          if (gf2k_xor2d(C.p, ldc, a, la, b, lb, rows, words, nullptr) != hipSuccess) FAIL("xor2d status");
          check(C, want, "xor2d", words, rows, mode, g);
          ++cases;
        }
    }
  return cases;
}

// gf2k_padcopy.  mul_strassen_padded (mul_dev_host.cpp) pads UP: drows >= srows, dwords >= the source's words; the source is a
// caller's view (any ld, any base), the destination its scratch.
static long run_padcopy() {
  long cases = 0;
  for (int scols : kCols)
    for (int srows : kRowsNarrow) {
      const int swords = wordsof(scols);
      if (srows == 300 && swords > 3) continue;
      for (int g = 0; g < 2 * 3 * 3 * 3 * 4; ++g) {
        const int drows = srows + 3 * (g & 1), dwords = swords + g / 2 % 3, dd = g / 6 % 3, ds = g / 18 % 3, od = g / 54 & 1, os = g / 108 & 1;
        const long long ldd = dwords + dd, lds_ = swords + ds;
        Words D(span(drows, ldd, dwords), 8 * od), S(span(srows, lds_, swords), 8 * os);
        std::vector<u64> want = D.snap();
        for (int r = 0; r < drows; ++r)
          for (int w = 0; w < dwords; ++w)
            want[r * ldd + w] = (r < srows && w < swords) ? (S[r * lds_ + w] & (w == swords - 1 ? lastmask(scols) : ~0ull)) : 0;
        if (gf2k_padcopy(D.p, ldd, drows, dwords, S.p, lds_, srows, scols, nullptr) != hipSuccess) FAIL("padcopy status");
        check(D, want, "padcopy", scols, srows, g);
        ++cases;
      }
    }
  return cases;
}

// gf2k_fill_random: word j of row r is splitmix64 of seed + ((row0 + r) * fullw + colw0 + j + 1) * golden, the last word under its mask
static long run_fill_random() {
  long cases = 0;
  for (int cols : kCols)
    for (int rows : kRowsNarrow) {
      const int w = wordsof(cols);
      if (rows == 300 && w > 3) continue;
      for (int g = 0; g < 3 * 2 * 3; ++g) {
        const long long ld = w + g % 3, row0 = (g / 6 % 3) * 1000003ll, fullw_in = g / 6 % 3 == 2 ? w + 5 : 0, colw0 = g / 6 % 3 == 2 ? 3 : 0;
        Words M(span(rows, ld, w), 8 * (g / 3 & 1));
        const u64 seed = rng();
        std::vector<u64> want = M.snap();
        const long long fullw = fullw_in > 0 ? fullw_in : w;
        for (int r = 0; r < rows; ++r)
          for (int j = 0; j < w; ++j) {
            u64 z = seed + ((u64)((row0 + r) * fullw + colw0 + j) + 1) * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            want[r * ld + j] = j == w - 1 ? z & lastmask(cols) : z;
          }
        if (gf2k_fill_random(M.p, ld, rows, cols, seed, row0, fullw_in, colw0, nullptr) != hipSuccess) FAIL("fill_random status");
        check(M, want, "fill_random", cols, rows, g);
        ++cases;
      }
    }
  return cases;
}

// gf2k_packA: word c of row r at ((r / 64) * wp + c) * 64 + r % 64; rows past m and words past w are zeros.  wp even, >= w (the
// launcher refuses anything else); the source is the caller's A: any ld, any base.
static long run_packA() {
  long cases = 0;
  const int ms[] = {1, 2, 63, 64, 65, 130};
  for (int m : ms)
    for (int w = 1; w <= 4; ++w)
      for (int g = 0; g < 2 * 3 * 2 * 2; ++g) {
        const long long wp = ((w + 1) & ~1) + 2 * (g & 1), lds_ = w + g / 2 % 3;
        const long long groups = (m + 63) / 64;
        Words D(groups * wp * 64, 8 * (g / 6 & 1)), S(span(m, lds_, w), 8 * (g / 12 & 1));
        std::vector<u64> want(D.n);
        for (long long r = 0; r < groups * 64; ++r)
          for (long long c = 0; c < wp; ++c) want[((r / 64) * wp + c) * 64 + r % 64] = (r < m && c < w) ? S[r * lds_ + c] : 0;
        if (gf2k_packA(D.p, wp, S.p, lds_, m, w, nullptr) != hipSuccess) FAIL("packA status");
        check(D, want, "packA", m, w, g);
        ++cases;
      }
  if (gf2k_packA(nullptr, 3, nullptr, 3, 1, 3, nullptr) == hipSuccess) FAIL("packA took an odd wp");
  return cases;
}

// gf2_splitk_reduce_kernel, launched as gf2k_m4rm launches it.  The partial products are the library's scratch: ldp even (gf2k_m4rm
// drops P otherwise), base 16-byte aligned, sP = m * ldp (apply_tile_plan, mul_dev_host.cpp).  C is the caller's: any ld, any base.
static long run_splitk_reduce() {
  long cases = 0;
  for (int words = 1; words <= 4; ++words)
    for (int m : kRowsNarrow) {
      if (m == 300 && words > 3) continue;
      for (int g = 0; g < 3 * 2 * 2 * 2 * 2; ++g) {
        const long long ldc = words + g % 3;
        const int oc = g / 3 & 1, acc = g / 6 & 1, batch = 1 + 2 * (g / 12 & 1), ksplit = 2 + 3 * (g / 24 & 1);
        const long long ldp = (words + 1) & ~1ll, sP = (long long)m * ldp, sC = (long long)m * ldc + 3;
        // the last slice of the last batch item ends with its last row's last PAIR: the kernel reads P in pairs, ldp is even
        Words P((long long)batch * ksplit * sP), C((batch - 1) * sC + span(m, ldc, words), 8 * oc);
        std::vector<u64> want = C.snap();
        for (int b = 0; b < batch; ++b)
          for (int r = 0; r < m; ++r)
            for (int w = 0; w < words; ++w) {
              u64 v = acc ? want[b * sC + r * ldc + w] : 0;
              for (int s = 0; s < ksplit; ++s) v ^= P[((long long)b * ksplit + s) * sP + r * ldp + w];
              want[b * sC + r * ldc + w] = v;
            }
        const long long total = (long long)m * ((words + 1) / 2) * batch;
        hipLaunchKernelGGL(gf2_splitk_reduce_kernel, dim3(grid_for(total)), dim3(256), 0, nullptr, C.p, ldc, sC, P.p, ldp, sP, ksplit, m,
                           words, batch, acc);
        check(C, want, "splitk_reduce", words, m, g);
        ++cases;
      }
    }
  return cases;
}

// gf2_streamk_reduce_kernel, launched as launch_v8 launches it: C (+)= the partial tiles of the last n_rem tiles.  Tile t is (row tile
// t % tiles_m, column tile t / tiles_m % tiles_n, batch item); its Q slabs are cut into segments of seg slabs (1 <= seg <= Q, so a
// segment spans two tiles at the most), segment s keeping its part of its first tile in slot 2 s and the rest in slot 2 s + 1.  Inside a
// slot of R * 8 words, the 16 bytes of piece k of row r lie at u64 index (((r % RPW) / 64 * 4 + (k ^ (r & 3))) * 512 + r / RPW * 64 +
// r % 64) * 2, RPW = 64 RG.  P is the library's scratch; C is the caller's: any ld, any base.
static long run_streamk_reduce() {
  long cases = 0;
  const int shapes[][3] = {{1, 1, 1}, {513, 65, 1}, {700, 512, 2}, {30, 600, 1}, {1025, 1000, 1}};  // m, n, batch
  for (int RG : {1, 2})
    for (const auto &sh : shapes)
      for (int g = 0; g < 3 * 2 * 2 * 3; ++g) {
        const int m = sh[0], n = sh[1], batch = sh[2], R = 512 * RG, RPW = 64 * RG, widthB = wordsof(n);
        const long long ldc = widthB + g % 3, sC = (long long)m * ldc + 1;
        const int oc = g / 3 & 1, acc = g / 6 & 1;
        gf2k_mul_args p{};
        p.tiles_m = (m + R - 1) / R, p.tiles_n = (n + 511) / 512;
        const int T = p.tiles_m * p.tiles_n * batch, Q = 5, seg = 1 + 2 * (g / 12);
        p.n_rem = g & 1 ? T : (T + 1) / 2, p.n_full = T - p.n_rem, p.tile_slabs = Q, p.seg_slabs = seg, p.nseg = (p.n_rem * Q + seg - 1) / seg;
        p.sP = (long long)R * 8, p.m = m, p.n = n, p.batch = batch, p.ldc = ldc, p.sC = sC, p.accumulate = acc;
        Words P(2ll * p.nseg * p.sP), C((batch - 1) * sC + span(m, ldc, widthB), 8 * oc);
        p.P = P.p, p.C = C.p;
        std::vector<u64> want = C.snap();
        for (int u = 0; u < p.n_rem; ++u) {
          const int t = p.n_full + u, tm = t % p.tiles_m, tn = t / p.tiles_m % p.tiles_n, bt = t / p.tiles_m / p.tiles_n;
          const long long glo = (long long)u * Q, ghi = glo + Q;
          for (int row = 0; row < R && tm * R + row < m; ++row)
            for (int j = 0; j < 8 && tn * 8 + j < widthB; ++j) {
              const long long e = ((long long)((row % RPW) / 64 * 4 + ((j >> 1) ^ (row & 3))) * 512 + row / RPW * 64 + row % 64) * 2 + (j & 1);
              u64 v = 0;
              for (long long s = glo / seg; s * seg < ghi && s < p.nseg; ++s) v ^= P[(2 * s + (s * seg < glo ? 1 : 0)) * p.sP + e];
              if (tn * 8 + j == widthB - 1) v &= lastmask(n);
              u64 &d = want[bt * sC + ((long long)tm * R + row) * ldc + tn * 8 + j];
              d = acc ? d ^ v : v;
            }
        }
        hipLaunchKernelGGL(gf2_streamk_reduce_kernel, dim3((unsigned)(p.n_rem * (R / 64))), dim3(256), 0, nullptr, p, RG);
        check(C, want, "streamk_reduce", RG, m, n, g);
        ++cases;
      }
  return cases;
}

static int parity(u64 x) { int p = 0; for (; x; x &= x - 1) p ^= 1; return p; }

// gf2k_rowparity: C (m x n) (+)= A (m x l) * Bt^T, one output word per thread, written whole (the bits past n as zeros, or kept when
// accumulating).  The launcher picks the register width from l and takes 16-byte loads of A only where lda and the base allow them.
static long run_rowparity() {
  long cases = 0;
  for (int l : {1, 63, 64, 65, 128, 129, 200, 256, 257, 512, 513})
    for (int m : {1, 3, 257})
      for (int n : {1, 64, 65, 130}) {
        if (m == 257 && (l > 129 || n > 65)) continue;
        for (int g = 0; g < 3 * 3 * 2 * 2 * 2; ++g) {
          if (g >= 18 && l > 257) continue;
          const int wl = wordsof(l), wn = wordsof(n), acc = g / 36;
          const long long lda = wl + g % 3, ldbt = wl + g / 3 % 3, ldc = wn + g % 2;
          Words A(span(m, lda, wl), 8 * (g / 9 & 1)), Bt(span(n, ldbt, wl), 8 * (g / 18 & 1)), C(span(m, ldc, wn), 8 * (g / 9 & 1));
          std::vector<u64> want = C.snap();
          for (int i = 0; i < m; ++i)
            for (int jw = 0; jw < wn; ++jw) {
              u64 out = 0;
              for (int j = 64 * jw; j < n && j < 64 * jw + 64; ++j) {
                u64 x = 0;
                for (int t = 0; t < wl; ++t) x ^= A[i * lda + t] & Bt[j * ldbt + t] & (t == wl - 1 ? lastmask(l) : ~0ull);
                out |= (u64)parity(x) << (j & 63);
              }
              want[i * ldc + jw] = acc ? want[i * ldc + jw] ^ out : out;
            }
          if (gf2k_rowparity(A.p, lda, Bt.p, ldbt, C.p, ldc, m, l, n, acc, nullptr) != hipSuccess) FAIL("rowparity status");
          check(C, want, "rowparity", l, m, n, g);
          ++cases;
        }
      }
  return cases;
}

// gf2k_packB (development builds only, tools/gf2_kernels_dev_thin.inc): dword d of rows 8 c .. 8 c + 7 of B -> the 32 bytes of lane d % 64 in block (tile d / 64, chunk
// c); rows past l, dwords past n's last and the padding chunks are zeros.  Bp is the tool's own allocation: 16-byte aligned.
static long run_packB() {
  long cases = 0;
  for (int l : {1, 8, 9, 33, 70})
    for (int n : {1, 31, 32, 33, 64, 65, 200, 2049})
      for (int g = 0; g < 3 * 2 * 2; ++g) {
        const int batch = 1 + 2 * (g / 6), nc = ((l + 31) / 32) * 4 + 4, tiles_n = (n + 2047) / 2048, wn = wordsof(n);
        const long long ldb = wn + g % 3, bStride = (long long)l * ldb + 1, bpStride = (long long)tiles_n * nc * 512 + 4 * (g / 3 & 1);
        Words B((batch - 1) * bStride + span(l, ldb, wn), 8 * (g / 3 & 1));
        Exact<u32> Bp((batch - 1) * bpStride + (long long)tiles_n * nc * 512);
        std::vector<u32> want = Bp.snap();
        for (int b = 0; b < batch; ++b)
          for (int tn = 0; tn < tiles_n; ++tn)
            for (int c = 0; c < nc; ++c)
              for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 8; ++r) {
                  const int row = 8 * c + r, d = tn * 64 + lane;
                  u32 x = 0;
                  if (row < l && d < 2 * wn) {
                    x = (u32)(B[b * bStride + row * ldb + d / 2] >> (32 * (d & 1)));
                    for (int bit = 0; bit < 32; ++bit)
                      if (32 * d + bit >= n) x &= ~(1u << bit);
                  }
                  want[b * bpStride + ((long long)tn * nc + c) * 512 + lane * 8 + r] = x;
                }
        if (gf2k_packB(Bp.p, bpStride, B.p, ldb, bStride, l, n, batch, nullptr) != hipSuccess) FAIL("packB status");
        for (long long i = 0; i < Bp.n; ++i)
          if (Bp[i] != want[i]) FAIL("packB l=%d n=%d g=%d dword %lld", l, n, g, i);
        ++cases;
      }
  return cases;
}

#endif  // EMU_STREAM
#ifdef EMU_STRASSEN
// --- Strassen passes.  mul_strassen (mul_dev_host.cpp) takes these passes only when every ld is even and every base 16-byte aligned,
// and the planner (mul_plan_host.cpp) only for leaf widths of an even word count: w even, h >= 1; the packed A side needs h % 64 == 0.
// Operands and products are dense (ld = w, stride = h * w); only the caller's matrix has an ld of its own.
static const int kSuppRef[2][7][2] = {  // quadrants (0 = X11, 1 = X12, 2 = X21, 3 = X22) of the combinations, from the formulas:
    {{0, 3}, {2, 3}, {0, -1}, {3, -1}, {0, 1}, {2, 0}, {1, 3}},   // A11+A22, A21+A22, A11, A22, A11+A12, A21+A11, A12+A22
    {{0, 3}, {0, -1}, {1, 3}, {2, 0}, {3, -1}, {0, 1}, {2, 3}}};  // B11+B22, B11, B12+B22, B21+B11, B22, B11+B12, B21+B22
static const int kFoldRef[4][4] = {{0, 3, 4, 6}, {2, 4, -1, -1}, {1, 3, -1, -1}, {0, 1, 2, 5}};  // C11, C12, C21, C22 from M1..M7

// word (r, c) of operand (q[0], .., q[L-1]) of a source of (h << L) rows x (w << L) words
static u64 split_ref(const u64 *X, long long ld, int L, int side, const int *q, int h, int w, long long r, long long c) {
  if (L == 0) return X[r * ld + c];
  u64 v = 0;
  for (int t = 0; t < 2; ++t) {
    const int quad = kSuppRef[side][q[0]][t];
    if (quad >= 0) v ^= split_ref(X, ld, L - 1, side, q + 1, h, w, r + (long long)(quad >> 1) * (h << (L - 1)), c + (long long)(quad & 1) * (w << (L - 1)));
  }
  return v;
}
// word (R, C) of the parent of 7^L products (dense h x w, one behind the other from M)
static u64 merge_ref(const u64 *M, int L, int h, int w, long long R, long long C, long long index) {
  if (L == 0) return M[index * h * w + R * w + C];
  const long long hh = (long long)h << (L - 1), ww = (long long)w << (L - 1);
  const int quad = (int)(R / hh) * 2 + (int)(C / ww);
  u64 v = 0;
  for (int t = 0; t < 4; ++t)
    if (kFoldRef[quad][t] >= 0) v ^= merge_ref(M, L - 1, h, w, R % hh, C % ww, index * 7 + kFoldRef[quad][t]);
  return v;
}

static long run_strassen_split(int L) {
  long cases = 0;
  const int shapes[][3] = {{1, 2, 0}, {2, 4, 0}, {3, 2, 0}, {1, 2, 1}, {2, 4, 1}, {64, 2, 2}, {128, 4, 2}, {64, 16, 2}};  // h, w, side
  const int ops = L == 1 ? 7 : L == 2 ? 49 : 343;
  for (const auto &sh : shapes) {
    const int h = sh[0], w = sh[1], kside = sh[2], side = kside == 2 ? 0 : kside;
    if (w == 16 && L != 3) continue;  // the tiled walk of the three-level pass alone
    for (int batch : {1, 3})
      for (int dl : {0, 2}) {
        if (w == 16 && (batch == 3 || dl)) continue;
        const long long H = (long long)h << L, W = (long long)w << L, lds_ = W + dl, srcStride = H * lds_, dstStride = (long long)h * w;
        Words X((batch - 1) * srcStride + span(H, lds_, W)), Y((long long)batch * ops * dstStride);
        std::vector<u64> want(Y.n);
        for (int b = 0; b < batch; ++b)
          for (int op = 0; op < ops; ++op) {
            int q[3];
            for (int k = L - 1, t = op; k >= 0; --k, t /= 7) q[k] = t % 7;
            for (int r = 0; r < h; ++r)
              for (int c = 0; c < w; ++c)
                want[((long long)b * ops + op) * dstStride + (kside == 2 ? ((long long)(r / 64) * w + c) * 64 + r % 64 : (long long)r * w + c)] =
                    split_ref(X.p + b * srcStride, lds_, L, side, q, h, w, r, c);
          }
        hipError_t e;
        const u64 *s0[1] = {X.p};
        if (L == 1) e = gf2k_strassen_split(Y.p, w, dstStride, X.p, lds_, srcStride, h, w, kside, batch, nullptr);
        else if (L == 2) e = gf2k_strassen_split2(Y.p, w, dstStride, X.p, lds_, srcStride, h, w, kside, batch, nullptr);
        else e = gf2k_strassen_split3(Y.p, w, dstStride, s0, nullptr, 1, lds_, srcStride, h, w, kside, batch, nullptr);
        if (e != hipSuccess) FAIL("strassen split status");
        check(Y, want, "strassen split", L, h, w, kside * 100 + batch * 10 + dl);
        ++cases;
      }
  }
  return cases;
}

// three levels under a virtual fourth (mul_strassen's split_step with st.virt): group g reads the XOR of one or two quadrants of the
// grandparent; operand (b, g, op) at ((b * 7 + g) * 343 + op) * dstStride
static long run_strassen_split3_virtual() {
  long cases = 0;
  const int shapes[][3] = {{1, 2, 0}, {2, 2, 1}, {64, 2, 2}};
  for (const auto &sh : shapes)
    for (int batch : {1, 3}) {
      const int h = sh[0], w = sh[1], kside = sh[2], side = kside == 2 ? 0 : kside;
      const long long hq = 8ll * h, wq = 8ll * w, lds_ = 2 * wq + 2, srcStride = 2 * hq * lds_, dstStride = (long long)h * w;
      Words X((batch - 1) * srcStride + span(2 * hq, lds_, 2 * wq)), Y((long long)batch * 7 * 343 * dstStride);
      const u64 *s0[7], *s1[7];
      for (int g = 0; g < 7; ++g) {
        const int a = kSuppRef[side][g][0], b = kSuppRef[side][g][1];
        s0[g] = X.p + (a >> 1) * hq * lds_ + (a & 1) * wq;
        s1[g] = b >= 0 ? X.p + (b >> 1) * hq * lds_ + (b & 1) * wq : nullptr;
      }
      std::vector<u64> want(Y.n);
      for (int b = 0; b < batch; ++b)
        for (int g = 0; g < 7; ++g)
          for (int op = 0; op < 343; ++op) {
            const int q[3] = {op / 49, op / 7 % 7, op % 7};
            for (int r = 0; r < h; ++r)
              for (int c = 0; c < w; ++c) {
                u64 v = split_ref(s0[g] + b * srcStride, lds_, 3, side, q, h, w, r, c);
                if (s1[g]) v ^= split_ref(s1[g] + b * srcStride, lds_, 3, side, q, h, w, r, c);
                want[(((long long)b * 7 + g) * 343 + op) * dstStride + (kside == 2 ? ((long long)(r / 64) * w + c) * 64 + r % 64 : (long long)r * w + c)] = v;
              }
          }
      if (gf2k_strassen_split3(Y.p, w, dstStride, s0, s1, 7, lds_, srcStride, h, w, kside, batch, nullptr) != hipSuccess) FAIL("split3 status");
      check(Y, want, "strassen split3 virtual", h, w, kside, batch);
      ++cases;
    }
  return cases;
}

static long run_strassen_merge(int L) {
  long cases = 0;
  const int shapes[][2] = {{1, 2}, {2, 4}, {3, 2}, {5, 6}};
  const int ops = L == 1 ? 7 : L == 2 ? 49 : 343;
  for (const auto &sh : shapes)
    for (int batch : {1, 3})
      for (int groups : {1, 7})
        for (int g = 0; g < 4; ++g) {
          if (groups == 7 && (L != 3 || g > 0)) continue;  // parents side by side: the three-level pass alone (dense parents, no accumulate)
          const int h = sh[0], w = sh[1], acc = groups == 7 ? 0 : g & 1, dl = groups == 7 ? 0 : 2 * (g >> 1), parents = batch * groups;
          const long long H = (long long)h << L, W = (long long)w << L, ldd = W + dl, dstStride = H * ldd, srcStride = (long long)h * w;
          Words M((long long)parents * ops * srcStride), C((parents - 1) * dstStride + span(H, ldd, W));
          std::vector<u64> want = C.snap();
          for (int p = 0; p < parents; ++p)
            for (long long R = 0; R < H; ++R)
              for (long long Cc = 0; Cc < W; ++Cc) {
                u64 &d = want[p * dstStride + R * ldd + Cc];
                d = (acc ? d : 0) ^ merge_ref(M.p + (long long)p * ops * srcStride, L, h, w, R, Cc, 0);
              }
          hipError_t e;
          if (L == 1) e = gf2k_strassen_merge(C.p, ldd, dstStride, M.p, w, srcStride, h, w, acc, batch, nullptr);
          else if (L == 2) e = gf2k_strassen_merge2(C.p, ldd, dstStride, M.p, w, srcStride, h, w, acc, batch, nullptr);
          else e = gf2k_strassen_merge3(C.p, ldd, dstStride, M.p, w, srcStride, h, w, acc, groups, batch, nullptr);
          if (e != hipSuccess) FAIL("strassen merge status");
          check(C, want, "strassen merge", L, h, w, batch * 100 + groups * 10 + g);
          ++cases;
        }
  return cases;
}

#endif  // EMU_STRASSEN
#ifdef EMU_REST
// ---------------------------------------------------------------------------------------------------------------------------------
// gf2_ple.hip, gf2_trsm.hip
// ---------------------------------------------------------------------------------------------------------------------------------
static unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }  // the host code's grid_of(n, 256)

// ple_panel_apply.  The table is what ple_panel_pivots leaves: built here with plain loops from a random word column (row rank
// profile in row order, then the column-greedy elimination of those rows).
static long run_panel_apply() {
  long cases = 0;
  const int cnts[] = {1, 2, 3, 5, 64, 65, 300}, widths[] = {1, 7, 63, 64};
  for (int cnt : cnts)
    for (int ncols : widths)
      for (int g = 0; g < 3 * 2 * 3; ++g) {
        const u64 vmask = lastmask(ncols);
        const long long lda = 1 + g % 3;
        Words col(cnt), tab(257), A(span(cnt, lda, 1), 8 * (g / 3 & 1));
        Exact<int> pi(cnt);
        const int density = g / 6;  // 0: random, 1: sparse (low rank), 2: zero column
        for (int i = 0; i < cnt; ++i) col[i] = density == 0 ? rng() : density == 1 ? (rng() & rng() & rng() & 0x11) : ~vmask;
        // row rank profile
        std::vector<u64> basis;
        std::vector<int> S;
        for (int i = 0; i < cnt; ++i) {
          u64 x = col[i] & vmask;
          for (u64 b : basis)
            if (x & (b & (~b + 1))) x ^= b;
          if (x) {
            for (u64 &b : basis)
              if (b & (x & (~x + 1))) b ^= x;
            basis.push_back(x);
            S.push_back(i);
          }
        }
        const int rank = (int)S.size();
        std::vector<u64> y(rank), E(rank);
        std::vector<int> pc(rank), prow(rank);
        std::vector<char> remaining(rank, 1);
        for (int k = 0; k < rank; ++k) y[k] = col[S[k]] & vmask;
        int k = 0;
        for (int c = 0; c < 64 && k < rank; ++c) {
          int p = -1;
          for (int j = 0; j < rank && p < 0; ++j)
            if (remaining[j] && ((y[j] >> c) & 1)) p = j;
          if (p < 0) continue;
          remaining[p] = 0;
          for (int j = 0; j < rank; ++j)
            if (remaining[j] && ((y[j] >> c) & 1)) y[j] ^= y[p];
          E[k] = y[p], pc[k] = c, prow[k] = S[p];
          ++k;
        }
        if (k != rank) FAIL("panel_apply driver: rank");
        for (int j = 0; j < rank; ++j) tab[j] = E[j], tab[64 + j] = (u64)pc[j], tab[128 + j] = (u64)prow[j];
        for (int j = 0; j < 64; ++j) tab[192 + j] = j < rank ? (u64)S[j] : ~0ull;
        tab[256] = (u64)rank;
        // expectation: pivot rows by pivot column, then the other rows in order; the word becomes the row's coordinates
        std::vector<u64> want = A.snap();
        std::vector<int> wantpi(cnt);
        std::vector<char> isS(cnt, 0);
        for (int s : S) isS[s] = 1;
        int next = 0;
        for (int i = 0; i < cnt; ++i) {
          int src;
          if (i < rank) src = prow[i];
          else {
            while (isS[next]) ++next;
            src = next++;
          }
          u64 x = col[src] & vmask, c = 0;
          for (int j = 0; j < rank; ++j)
            if ((x >> pc[j]) & 1) x ^= E[j], c |= 1ull << j;
          const u64 out = i < rank ? ((c & (i ? (~0ull >> (64 - i)) : 0)) | E[i]) : c;
          want[i * lda] = (want[i * lda] & ~vmask) | (out & vmask);
          wantpi[i] = src;
        }
        hipLaunchKernelGGL(ple_panel_apply, dim3(blocks_of(cnt)), dim3(256), 0, nullptr, col.p, cnt, vmask, tab.p, A.p, lda, pi.p);
        check(A, want, "panel_apply", cnt, ncols, g);
        for (int i = 0; i < cnt; ++i)
          if (pi[i] != wantpi[i]) FAIL("panel_apply pi cnt=%d ncols=%d g=%d i=%d", cnt, ncols, g, i);
        ++cases;
      }
  return cases;
}

// ple_gather: dst[i][w] = src[perm ? perm[i] : i][w] (src null: 0), the last word under lastmask
static long run_gather() {
  long cases = 0;
  for (int cols : kCols)
    for (int rows : kRowsNarrow) {
      const int words = wordsof(cols);
      if (rows == 300 && words > 3) continue;
      for (int g = 0; g < 3 * 3 * 2 * 2 * 3; ++g) {
        const long long ldd = words + g % 3, lds_ = words + g / 3 % 3;
        const int mode = g / 36;  // 0: permutation, 1: identity (perm null), 2: zero (src null, ld 0)
        const u64 lm = (g / 9 & 1) ? ~0ull : lastmask(cols);
        Words D(span(rows, ldd, words), 8 * (g / 18 & 1)), S(span(rows, lds_, words), 8 * (g / 9 & 1));
        Exact<int> perm(rows);
        for (int i = 0; i < rows; ++i) perm[i] = i;
        for (int i = rows - 1; i > 0; --i) std::swap(perm[i], perm[rng() % (i + 1)]);
        std::vector<u64> want = D.snap();
        for (int i = 0; i < rows; ++i)
          for (int w = 0; w < words; ++w) {
            const u64 m = w == words - 1 ? lm : ~0ull, v = mode == 2 ? 0 : S[(mode == 0 ? perm[i] : i) * lds_ + w];
            want[i * ldd + w] = (want[i * ldd + w] & ~m) | (v & m);
          }
        hipLaunchKernelGGL(ple_gather, dim3(blocks_of((long long)rows * words)), dim3(256), 0, nullptr, D.p, ldd,
                           mode == 2 ? (const u64 *)nullptr : S.p, mode == 2 ? 0ll : lds_, mode == 0 ? perm.p : (const int *)nullptr, rows,
                           words, lm);
        check(D, want, "gather", cols, rows, g);
        ++cases;
      }
    }
  return cases;
}

static long run_compose() {
  long cases = 0;
  for (int cnt : {1, 2, 255, 256, 257, 700})
    for (int r1 : {0, 1, 64}) {
      Exact<int> pi(cnt), stash(r1 + cnt);
      for (int i = 0; i < cnt; ++i) pi[i] = i;
      for (int i = cnt - 1; i > 0; --i) std::swap(pi[i], pi[rng() % (i + 1)]);
      std::vector<int> want(cnt);
      for (int j = 0; j < cnt; ++j) want[j] = stash[r1 + pi[j]];
      hipLaunchKernelGGL(ple_compose, dim3(blocks_of(cnt)), dim3(256), 0, nullptr, pi.p, stash.p, r1, cnt);
      for (int j = 0; j < cnt; ++j)
        if (pi[j] != want[j]) FAIL("compose cnt=%d r1=%d j=%d", cnt, r1, j);
      ++cases;
    }
  return cases;
}

// ple_compress_extract / ple_compress_place with the parameters ple_rec computes for a node [c0, c1) of `rest` remaining rows:
// cmid = c0 + 64 * ceil(words / 2), ranks r1 <= cmid - c0 and r2 <= min(rest, c1 - cmid), launched when r2 > 0 and r1 < cmid - c0.
// The matrix ends with the node (c1 = n), so each row's last word is the node's and the buffer ends with it.
//
// INVARIANT of the shipped caller: sbit = cmid is a multiple of 64 (c0 is 0 or an ancestor's cmid).  The extract is driven with other
// sbit as well (stand-alone, below): the kernel loads row[w + 1] only when the wanted bits reach into it, so the row's last word may be
// the buffer's last for any sbit.
static long run_compress() {
  long cases = 0;
  for (int c0 : {0, 64, 128})
    for (int width : {65, 100, 128, 129, 200, 257}) {
      const int c1 = c0 + width, cmid = c0 + 64 * ((wordsof(width) + 1) / 2), nw = wordsof(c1);
      for (int rest : {1, 2, 5, 70, 140})
        for (int r1 : {0, 1, 37, cmid - c0 - 1})
          for (int r2 : {1, 2, 63, 64, 65, std::min(rest, c1 - cmid)}) {
            if (r2 > std::min(rest, c1 - cmid) || r1 >= cmid - c0) continue;
            for (int dl = 0; dl < 3; ++dl) {
              const long long lda = nw + dl;
              const int sw = wordsof(r2), dbit = c0 + r1, wlo = dbit >> 6, whi = wordsof(cmid + r2);
              Words A(span(rest, lda, nw), 8 * (dl & 1)), S((long long)rest * sw);
              const std::vector<u64> a0 = A.snap();
              hipLaunchKernelGGL(ple_compress_extract, dim3(blocks_of((long long)rest * sw)), dim3(256), 0, nullptr, A.p, lda, rest, cmid, r2,
                                 S.p, sw);
              check(A, a0, "compress_extract changed A", c0, width, rest, r1 * 1000 + r2);
              for (int i = 0; i < rest; ++i)
                for (int b = 0; b < sw * 64; ++b)
                  if (getbit(S.p + (long long)i * sw, b) != (b < std::min(i, r2) ? getbit(a0.data() + i * lda, cmid + b) : 0))
                    FAIL("compress_extract c0=%d width=%d rest=%d r1=%d r2=%d row %d bit %d", c0, width, rest, r1, r2, i, b);
              std::vector<u64> want = a0;
              for (int i = 0; i < rest; ++i) {
                const int wi = std::min(i, r2);
                u64 *row = want.data() + i * lda;
                for (int b = 0; b < wi; ++b) row[(cmid + b) >> 6] &= ~(1ull << ((cmid + b) & 63));
                for (int b = 0; b < wi; ++b) row[(dbit + b) >> 6] |= (u64)getbit(a0.data() + i * lda, cmid + b) << ((dbit + b) & 63);
              }
              hipLaunchKernelGGL(ple_compress_place, dim3(blocks_of((long long)rest * (whi - wlo))), dim3(256), 0, nullptr, A.p, lda, rest, cmid,
                                 dbit, r2, S.p, sw, wlo, whi - wlo);
              check(A, want, "compress_place", c0, width, rest, r1 * 1000 + r2);
              ++cases;
            }
          }
    }
  // the extract at any sbit: the wanted bits [sbit, sbit + min(i, r2)) end with the row, the row with the buffer
  for (int sbit : {1, 31, 63, 64, 65, 100, 127})
    for (int r2 : {1, 2, 28, 63, 64, 65, 130})
      for (int rest : {1, 3, 70, 140}) {
        const int ncols = sbit + std::min(rest - 1 > 0 ? rest - 1 : 1, r2), nw = wordsof(ncols), sw = wordsof(r2);
        for (int dl = 0; dl < 3; ++dl) {
          const long long lda = nw + dl;
          Words A(span(rest, lda, nw), 8 * (dl & 1)), S((long long)rest * sw);
          const std::vector<u64> a0 = A.snap();
          hipLaunchKernelGGL(ple_compress_extract, dim3(blocks_of((long long)rest * sw)), dim3(256), 0, nullptr, A.p, lda, rest, sbit, r2, S.p, sw);
          check(A, a0, "compress_extract changed A", sbit, r2, rest, dl);
          for (int i = 0; i < rest; ++i)
            for (int b = 0; b < sw * 64; ++b)
              if (getbit(S.p + (long long)i * sw, b) != (b < std::min(i, r2) ? getbit(a0.data() + i * lda, sbit + b) : 0))
                FAIL("compress_extract sbit=%d r2=%d rest=%d row %d bit %d", sbit, r2, rest, i, b);
          ++cases;
        }
      }
  return cases;
}

// ple_tri (mode 0: dst = src without the bits below the diagonal and past ncols; mode 1: dst keeps those, takes the others) and
// trsm_copy_back (dst = src, the last word under its mask)
static long run_tri_copy_back(int which) {
  long cases = 0;
  for (int cols : kCols)
    for (int rows : kRowsNarrow) {
      const int words = wordsof(cols);
      if (rows == 300 && words > 3) continue;
      if (which < 2 && rows > cols) continue;  // ple_tri's rows are the rank: r <= n
      for (int g = 0; g < 3 * 3 * 2 * 2; ++g) {
        const long long ldd = words + g % 3, lds_ = words + g / 3 % 3;
        Words D(span(rows, ldd, words), 8 * (g / 9 & 1)), S(span(rows, lds_, words), 8 * (g / 18 & 1));
        std::vector<u64> want = D.snap();
        for (int j = 0; j < rows; ++j)
          for (long long c = 0; c < words * 64; ++c) {
            const int s = getbit(S.p + j * lds_, c), d = getbit(want.data() + j * ldd, c);
            int v;
            if (which == 0) v = (c >= j && c < cols) ? s : 0;
            else if (which == 1) v = (c >= j && c < cols) ? s : d;
            else v = c < cols ? s : d;
            want[j * ldd + (c >> 6)] = (want[j * ldd + (c >> 6)] & ~(1ull << (c & 63))) | ((u64)v << (c & 63));
          }
        if (which < 2)
          hipLaunchKernelGGL(ple_tri, dim3(blocks_of((long long)rows * words)), dim3(256), 0, nullptr, D.p, ldd, S.p, lds_, rows, words,
                             lastmask(cols), which);
        else
          hipLaunchKernelGGL(trsm_copy_back, dim3(blocks_of((long long)rows * words)), dim3(256), 0, nullptr, D.p, ldd, S.p, lds_, rows, words,
                             lastmask(cols));
        check(D, want, which < 2 ? "tri" : "copy_back", cols, rows, g, which);
        ++cases;
      }
    }
  return cases;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gf2_nullspace.hip: nullspace_prepare + nullspace_assemble, launched as gf2_nullspace_dev launches them.  K by the definition in the
// file's header: row f_j = e_j, row p_i = the bits of E's row i at the free columns, in order.  E: r rows (the rows below hold no pivot
// and are not read), the buffer ends with row r - 1.
// ---------------------------------------------------------------------------------------------------------------------------------
static long run_nullspace() {
  long cases = 0;
  for (int n : {1, 63, 64, 65, 128, 129, 200, 513}) {
    std::vector<std::vector<int>> sets;
    auto add = [&](auto pred) {
      std::vector<int> p;
      for (int c = 0; c < n; ++c)
        if (pred(c)) p.push_back(c);
      if ((int)p.size() < n) sets.push_back(p);  // d = 0: gf2_nullspace_dev returns before any launch
    };
    add([](int) { return false; });                      // none
    add([&](int c) { return c != 0; });                  // all but one column: the first, the last, one in the middle
    add([&](int c) { return c != n - 1; });
    add([&](int c) { return c != n / 2; });
    add([&](int c) { return c < n / 2; });               // pivots first
    add([&](int c) { return c < n - 1 && c < 64; });
    add([&](int c) { return c >= n - n / 2; });          // pivots last
    add([](int c) { return (c & 1) == 0; });             // alternating
    add([](int c) { return (c & 1) == 1; });
    add([](int c) { return c < 128 && (c & 1); });       // free index 64 is column 128: the first bit of a source word
    add([](int c) { return c < 127 && (c & 1); });       // free index 64 is column 127: the last bit of a source word
    add([](int c) { return c < 191 && c >= 64 && (c & 1); });  // free index 128 is column 191 (64 free columns, then 64 among 64..190)
    add([&](int) { return rng() % 3 == 0; });             // random
    for (const auto &piv : sets)
      for (int g = 0; g < 4; ++g) {
        const int r = (int)piv.size(), d = n - r, nw = wordsof(n), kw = wordsof(d);
        const long long lde = nw + (g & 1), ldk = kw + (g >> 1);
        Exact<int> pivcols(r), rowinfo(n);
        for (int i = 0; i < r; ++i) pivcols[i] = piv[i];
        Words E(span(r, lde, nw), 8 * (g & 1)), K(span(n, ldk, kw), 8 * (g >> 1)), fmask(nw), ctl((long long)nw * CTL_WORDS);
        Exact<int2> start(kw);
        std::vector<int> freecols;
        std::vector<char> isp(n, 0);
        for (int c : piv) isp[c] = 1;
        for (int c = 0; c < n; ++c)
          if (!isp[c]) freecols.push_back(c);
        std::vector<u64> want = K.snap();
        for (int c = 0; c < n; ++c)
          for (int w = 0; w < kw; ++w) want[c * ldk + w] = 0;
        for (int j = 0; j < d; ++j) want[freecols[j] * ldk + (j >> 6)] |= 1ull << (j & 63);
        for (int i = 0; i < r; ++i)
          for (int j = 0; j < d; ++j) want[piv[i] * ldk + (j >> 6)] |= (u64)getbit(E.p + i * lde, freecols[j]) << (j & 63);
        // the launch shapes of gf2_nullspace_dev
        int wx = 1;
        while (wx < kw && wx < 256) wx <<= 1;
        const int ry = 256 / wx;
        hipLaunchKernelGGL(nullspace_prepare, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, nullptr, pivcols.p, r, n, nw, kw, fmask.p,
                           ctl.p, rowinfo.p, start.p);
        for (int q = 0; q < nw; ++q) {
          u64 fm = 0;
          for (int b = 0; b < 64 && q * 64 + b < n; ++b) fm |= (u64)!isp[q * 64 + b] << b;
          if (fmask[q] != fm) FAIL("nullspace fmask n=%d r=%d q=%d", n, r, q);
        }
        for (int c = 0, i = 0, j = 0; c < n; ++c)
          if (rowinfo[c] != (isp[c] ? i++ : ~(j++))) FAIL("nullspace rowinfo n=%d r=%d c=%d", n, r, c);
        for (int w = 0; w < kw; ++w) {
          const int c = freecols[w * 64];
          int before = 0;
          for (int b = 0; b < (c & 63); ++b) before += !isp[(c & ~63) + b];
          if (start[w].x != (c >> 6) || start[w].y != before) FAIL("nullspace start n=%d r=%d w=%d", n, r, w);
        }
        hipLaunchKernelGGL(nullspace_assemble, dim3((unsigned)((n + ry - 1) / ry), (unsigned)((kw + wx - 1) / wx)), dim3(wx, ry), 0, nullptr,
                           E.p, lde, nw, fmask.p, ctl.p, rowinfo.p, start.p, K.p, ldk, n, kw, d);
        check(K, want, "nullspace", n, r, g);
        ++cases;
        // The walk over the source words ends with the last of them, whatever it is asked for.  With consistent arguments it ends
        // sooner (the free bits from the start entry on are exactly the bits the output words need), so the bound `q < nw` shows only
        // when d overstates the free columns by one: the row's last word then comes out with a zero there, and no mask past the nw-th
        // is read.
        if (d & 63) {
          for (long long i = 0; i < K.n; ++i) K[i] = rng();
          std::vector<u64> want2 = K.snap();
          for (int c = 0; c < n; ++c)
            for (int w = 0; w < kw; ++w) want2[c * ldk + w] = want[c * ldk + w];
          hipLaunchKernelGGL(nullspace_assemble, dim3((unsigned)((n + ry - 1) / ry), (unsigned)((kw + wx - 1) / wx)), dim3(wx, ry), 0, nullptr,
                             E.p, lde, nw, fmask.p, ctl.p, rowinfo.p, start.p, K.p, ldk, n, kw, d + 1);
          check(K, want2, "nullspace, d + 1", n, r, g);
          ++cases;
        }
      }
  }
  return cases;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gf2_elim.hip: the row moves of a block's end, the toggle, and the three launchers
// ---------------------------------------------------------------------------------------------------------------------------------
static long run_elim_moves() {
  long cases = 0;
  for (int nmoves : {0, 1, 5, 300})
    for (int nA : {1, 2, 255, 256, 257})
      for (int uw : {0, 1, 3})
        for (int g = 0; g < 4; ++g) {
          if (nA > 2 && (g == 1 || g == 2 || (g && nmoves == 300))) continue;  // each launch walks the library's 4096 workgroups
          const int m = nmoves + 7;
          const long long c0w = g & 1, aw = c0w + nA, lda = aw + (g >> 1), ldu = uw + (g >> 1), tld = nA + uw + (g & 1);
          Words A(span(m, lda, aw), 8 * (g & 1)), U(uw ? span(m, ldu, uw) : 0, 8 * (g >> 1)), T(span(nmoves, tld, nA + uw));
          Exact<int> moves(4 * GF2K_ELIM_BLOCK_PIVOTS);
          Exact<gf2k_elim_state> st(1);
          st[0].nmoves = nmoves;
          std::vector<int> from(m), to(m);
          for (int i = 0; i < m; ++i) from[i] = to[i] = i;
          for (int i = m - 1; i > 0; --i) std::swap(from[i], from[rng() % (i + 1)]), std::swap(to[i], to[rng() % (i + 1)]);
          for (int q = 0; q < nmoves; ++q) moves[q] = from[q], moves[2 * GF2K_ELIM_BLOCK_PIVOTS + q] = to[q];
          std::vector<u64> wantT = T.snap(), wantA = A.snap(), wantU = U.snap();
          for (int q = 0; q < nmoves; ++q)
            for (int w = 0; w < nA + uw; ++w) wantT[q * tld + w] = w < nA ? A[from[q] * lda + c0w + w] : U[from[q] * ldu + w - nA];
          u64 *Up = uw ? U.p : nullptr;
          hipLaunchKernelGGL(gf2_elim_gather_kernel, dim3(2 * GF2K_ELIM_BLOCK_PIVOTS), dim3(256), 0, nullptr, A.p, lda, aw, c0w, Up, ldu, uw,
                             st.p, moves.p, T.p, tld);
          check(T, wantT, "elim_gather", nmoves, nA, uw, g);
          for (int q = 0; q < nmoves; ++q)
            for (int w = 0; w < nA + uw; ++w) (w < nA ? wantA[to[q] * lda + c0w + w] : wantU[to[q] * ldu + w - nA]) = wantT[q * tld + w];
          hipLaunchKernelGGL(gf2_elim_scatter_kernel, dim3(2 * GF2K_ELIM_BLOCK_PIVOTS), dim3(256), 0, nullptr, A.p, lda, aw, c0w, Up, ldu, uw,
                             st.p, moves.p, T.p, tld);
          check(A, wantA, "elim_scatter A", nmoves, nA, uw, g);
          check(U, wantU, "elim_scatter U", nmoves, nA, uw, g);
          ++cases;
        }
  return cases;
}

static long run_elim_small() {
  long cases = 0;
  // toggle: U'[r0 + j][j] ^= 1 for the block's pivots j < r_cur - r0; the matrix ends with row r_cur - 1
  for (int r0 : {0, 3, 100})
    for (int np : {0, 1, 63, 64, 65, 300, GF2K_ELIM_BLOCK_PIVOTS})
      for (int dl = 0; dl < 3; ++dl) {
        const int uw = wordsof(np ? np : 1);
        const long long ldu = uw + dl;
        Words U(span(r0 + np, ldu, uw), 8 * (dl & 1));
        Exact<gf2k_elim_state> st(1);
        st[0].r0 = r0, st[0].r_cur = r0 + np;
        std::vector<u64> want = U.snap();
        for (int j = 0; j < np; ++j) want[(r0 + j) * ldu + (j >> 6)] ^= 1ull << (j & 63);
        hipLaunchKernelGGL(gf2_elim_toggle_kernel, dim3(GF2K_ELIM_BLOCK_PIVOTS / 256), dim3(256), 0, nullptr, U.p, ldu, st.p);
        check(U, want, "elim_toggle", r0, np, dl);
        ++cases;
      }
  // gf2k_set_diag: M[i][col0 + i] = 1; the matrix ends with the word of its last diagonal bit
  for (int n : {1, 2, 63, 64, 65, 300})
    for (long long col0 : {0ll, 1ll, 63ll, 64ll, 100ll})
      for (int dl = 0; dl < 3; ++dl) {
        const int w = wordsof(col0 + n);
        const long long ld = w + dl;
        Words M(span(n, ld, w), 8 * (dl & 1));
        std::vector<u64> want = M.snap();
        for (int i = 0; i < n; ++i) want[i * ld + ((col0 + i) >> 6)] |= 1ull << ((col0 + i) & 63);
        if (gf2k_set_diag(M.p, ld, n, col0, nullptr) != hipSuccess) FAIL("set_diag status");
        check(M, want, "set_diag", n, col0, dl);
        ++cases;
      }
  // gf2k_scatter_rows: X[pivcols[k]] = R[k]
  for (int words : {1, 2, 255, 256, 257})
    for (int rank : {1, 2, 5, 70})
      for (int g = 0; g < 9; ++g) {
        const int nx = rank + 5;
        const long long ldx = words + g % 3, ldr = words + g / 3;
        Words X(span(nx, ldx, words), 8 * (g & 1)), R(span(rank, ldr, words), 8 * (g / 3 & 1));
        Exact<int> piv(rank);
        std::vector<int> rows(nx);
        for (int i = 0; i < nx; ++i) rows[i] = i;
        for (int i = nx - 1; i > 0; --i) std::swap(rows[i], rows[rng() % (i + 1)]);
        std::sort(rows.begin(), rows.begin() + rank);
        std::vector<u64> want = X.snap();
        for (int k = 0; k < rank; ++k) {
          piv[k] = rows[k];
          for (int w = 0; w < words; ++w) want[rows[k] * ldx + w] = R[k * ldr + w];
        }
        if (gf2k_scatter_rows(X.p, ldx, R.p, ldr, words, piv.p, rank, nullptr) != hipSuccess) FAIL("scatter_rows status");
        check(X, want, "scatter_rows", words, rank, g);
        ++cases;
      }
  // gf2k_elim_begin_block: one thread writes six fields, the others stay
  {
    Exact<gf2k_elim_state> st(1);
    gf2k_elim_state want = st[0];
    want.r0 = want.scan = want.r_cur, want.np = 0, want.lastword = -1, want.cntP = want.cnt2 = 0;
    g_block_threads = 64;
    if (gf2k_elim_begin_block(st.p, nullptr) != hipSuccess) FAIL("begin_block status");
    g_block_threads = 256;
    if (memcmp(&want, st.p, sizeof want)) FAIL("elim_begin_block");
    ++cases;
  }
  return cases;
}

#endif  // EMU_REST

int main() {
#define RUN(name, call)                               \
  do {                                                \
    const long n_ = call;                             \
    printf("%s: %ld cases ok\n", name, n_);           \
    fflush(stdout);                                   \
  } while (0)
#ifdef EMU_STREAM
  RUN("gf2_xor2d_kernel", run_xor2d());
  RUN("gf2_padcopy_kernel", run_padcopy());
  RUN("gf2_fill_random_kernel", run_fill_random());
  RUN("gf2_packA_kernel", run_packA());
  RUN("gf2_splitk_reduce_kernel", run_splitk_reduce());
  RUN("gf2_streamk_reduce_kernel", run_streamk_reduce());
  RUN("gf2_rowparity_kernel", run_rowparity());
  RUN("gf2_packB_kernel", run_packB());
#endif
#ifdef EMU_STRASSEN
  RUN("gf2_strassen_split_kernel", run_strassen_split(1));
  RUN("gf2_strassen_split2_kernel", run_strassen_split(2));
  RUN("gf2_strassen_split3_kernel", run_strassen_split(3) + run_strassen_split3_virtual());
  RUN("gf2_strassen_merge_kernel", run_strassen_merge(1));
  RUN("gf2_strassen_merge2_kernel", run_strassen_merge(2));
  RUN("gf2_strassen_merge3_kernel", run_strassen_merge(3));
#endif
#ifdef EMU_REST
  RUN("ple_panel_apply", run_panel_apply());
  RUN("ple_gather", run_gather());
  RUN("ple_compose", run_compose());
  RUN("ple_compress_extract + ple_compress_place", run_compress());
  RUN("ple_tri", run_tri_copy_back(0) + run_tri_copy_back(1));
  RUN("trsm_copy_back", run_tri_copy_back(2));
  RUN("nullspace_prepare + nullspace_assemble", run_nullspace());
  RUN("gf2_elim_gather_kernel + gf2_elim_scatter_kernel", run_elim_moves());
  RUN("gf2_elim_toggle_kernel + gf2_set_diag_kernel + gf2_scatter_rows_kernel + gf2_elim_begin_block_kernel", run_elim_small());
#endif
  printf("all ok, %ld threads emulated\n", g_threads);
  return 0;
}
