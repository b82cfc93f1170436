// mul_dev_host.cpp -- the products on device matrices: executes what the launch planner (mul_plan_host.cpp) chose -- planned tile
// launches, the plain, Strassen, padded, peeled and naive products -- and gf2_mul_dev, gf2_mul_nt_dev, add, transpose, equal.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "dev_args.h"
#include "gf2_kernels.h"
#include "mul_plan.h"

typedef uint64_t u64;

// the host (mzd_t) entry points run on a private stream and wait for their product (sync_free); the device API never waits
static int sync_if(bool sync_free, hipStream_t s) {
  return sync_free && hipStreamSynchronize(s) != hipSuccess ? gf2_fail_hip(hipGetLastError(), "hipStreamSynchronize") : 0;
}
static int launch_m4rm(gf2k_mul_args a, int cfg, hipStream_t s) {
  HIP_TRY(gf2k_m4rm(a, cfg, s));
  return 0;
}

// fills in the launch fields of `a` from a plan (scratch for partial tiles from the stream's workspace slot 1); falls back to an
// unsplit launch when the scratch cannot be had
static int apply_tile_plan(gf2k_mul_args &a, const TilePlan &tp, hipStream_t s) {
  a.ksplit = 1;
  a.n_rem = a.nseg = 0;
  a.P = nullptr;
  a.p_words = 0;
  const size_t want = tp.scratch();  // (the launches of a plan run one after the other)
  if (want == 0) return 0;
  void *ws = nullptr;
  if (gf2_stream_scratch(s, want, &ws, GF2_SLOT_PARTIAL_TILES) != 0) return 0;
  a.P = static_cast<u64 *>(ws);
  a.p_words = (long long)(want / sizeof(u64));
  if (tp.ws_bytes == 0) return 0;
  if (gf2_variant_of(tp.cfg).v8_rg) {
    a.n_rem = tp.n_rem;
    a.nseg = tp.nseg;
  } else {
    a.ksplit = tp.ksplit;
    a.ldp = (words_of(a.n) + 1) & ~1ll;
    a.sP = (long long)a.m * a.ldp;
  }
  return 0;
}

// one planned (batched) product: the launch, and the launch of the tail products if the plan cuts the batch in two
static int launch_planned(gf2k_mul_args a, const TilePlan &tp, hipStream_t s) {
  ProfScope prof(s);
  const int total = a.batch;
  const int band = tp.band_rows > 0 && tp.band_rows < a.m ? tp.band_rows : 0;
  const gf2k_mul_args whole = a;
  a.m -= band;
  const bool cut = tp.tail_batch > 0 && tp.tail_batch < total;
  if (cut) a.batch = total - tp.tail_batch;
  if (int rc = apply_tile_plan(a, tp, s)) return rc;
  if (int rc = launch_m4rm(a, tp.cfg, s)) return rc;
  if (cut) {
    gf2k_mul_args b = a;
    const long long b1 = a.batch;
    b.A += b1 * a.sA;
    b.B += b1 * a.sB;
    b.C += b1 * a.sC;
    b.batch = tp.tail_batch;
    b.ksplit = 1;
    b.n_rem = b.P ? tp.tail.n_rem : 0;
    b.nseg = b.P ? tp.tail.nseg : 0;
    if (int rc = launch_m4rm(b, tp.tail.cfg, s)) return rc;
  }
  if (!band) return 0;
  // the row band: rows [m - band, m) of every product (m - band is a multiple of 2048, so the offset is the same
  // expression for row-major and row-group-packed A)
  gf2k_mul_args r = whole;
  r.A += (long long)a.m * whole.lda;
  r.C += (long long)a.m * whole.ldc;
  r.m = band;
  r.ksplit = 1;
  r.P = a.P;
  r.p_words = a.p_words;
  r.n_rem = r.P ? tp.band.n_rem : 0;
  r.nseg = r.P ? tp.band.nseg : 0;
  return launch_m4rm(r, tp.band.cfg, s);
}

static int mul_widevec(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, hipStream_t s) {
  const int m = A->nrows, l = A->ncols, n = B->ncols;
  const long long ldbt = (words_of(l) + 1) & ~1ll;
  void *bt = nullptr;
  if (int rc = gf2_stream_scratch(s, (size_t)n * ldbt * sizeof(u64), &bt, GF2_SLOT_OPERANDS)) return rc;
  HIP_TRY(gf2k_transpose(static_cast<u64 *>(bt), ldbt, B->data, B->ld, l, n, s));
  const u64 *Bt = static_cast<const u64 *>(bt);
  const int n0 = n < 32 ? n : 32;
  HIP_TRY(gf2k_widevec(A->data, A->ld, Bt, ldbt, C->data, C->ld, m, l, n0, accumulate, 0, s));
  if (n > 32) HIP_TRY(gf2k_widevec(A->data, A->ld, Bt + 32 * ldbt, ldbt, C->data, C->ld, m, l, n - 32, 1, 32, s));
  return 0;
}

int gf2_mul_m4rm_plain(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, hipStream_t s) {
  const int m = A->nrows, l = A->ncols, n = B->ncols;
  const PlainPath path = plain_path(m, l, n);
  if (path == kPathNothing) return 0;
  if (path == kPathZeroInner) {
    if (!accumulate) HIP_TRY(gf2k_xor2d(C->data, C->ld, nullptr, 0, nullptr, 0, m, words_of(n), s));
    return 0;
  }
  if (path == kPathSlabTables) {
    HIP_TRY(gf2k_tallskinny_long(A->data, A->ld, B->data, B->ld, C->data, C->ld, m, l, n, accumulate, s));
    return 0;
  }
  // 65-128 columns against a long inner dimension: that kernel with 16-byte entries, where the tile kernel finds a single column
  // tile and a handful of row tiles (65536^2 x 128: 0.78 -> 0.27 ms; 20000^2 x 128: 143 -> 46 us; 9000 x 33000 x 100: 126 -> 37 us).
  // A second pass for 129-256 columns pays from 32768-bit rows on (65536^2 x 256: 0.78 -> 0.53 ms; 65536 x 8192 x 256: 98 -> 125 us).
  if (path == kPathSlabPasses) {
    for (int c0 = 0; c0 < n; c0 += 128)
      HIP_TRY(gf2k_tallskinny_long(A->data, A->ld, B->data + c0 / 64, B->ld, C->data + c0 / 64, C->ld, m, l, std::min(128, n - c0), accumulate, s));
    return 0;
  }
  if (path == kPathWideVec) return mul_widevec(C, A, B, accumulate, s);  // few columns, long rows: a wave per row
  // tall and skinny: tables over ALL of B, A streamed once.  Built for short inner dimensions (a batch of LPN samples: l = 256);
  // with a long one the tables are rebuilt every 256 bits and the tile kernel with split-K is ~10x faster (65536 x 65600 x 64:
  // 6.4 ms here), so the border strips of peeled products do not come this way
  if (path == kPathTallSkinny) {
    HIP_TRY(gf2k_tallskinny(A->data, A->ld, B->data, B->ld, C->data, C->ld, m, l, n, accumulate, s));
    return 0;
  }
  if (path == kPathFewRows) {  // a handful of rows: stream B once (v*A path, binary_matrix.rs:552-563)
    if (!accumulate) HIP_TRY(gf2k_xor2d(C->data, C->ld, nullptr, 0, nullptr, 0, m, words_of(n), s));
    HIP_TRY(gf2k_va(A->data, A->ld, B->data, B->ld, C->data, C->ld, m, l, n, s));
    return 0;
  }
  // 9 to 128 rows against a tall B: the tile kernel would build its 256-entry tables for a handful of rows (64 x 65536 x 4096:
  // 90 us; 16 x 200000 x 600: 144 us for 15 MB of B).  Transposed, the product is n rows of l bits times at most 64 vectors per
  // pass -- the slab table kernel's shape: C^T = B^T A^T, with B transposed once (one more pass over B) and the small operands
  // transposed in and out.  Only for a B much taller than wide: the transposition of B runs at 1.7-1.9 TB/s (64 x 20000 x 20000:
  // 93 -> 151 us, 64 x 65536 x 65536: 0.86 -> 0.81 ms).
  {
    if (path == kPathFewRowsT) {
      const int passes = (m + 63) / 64;
      const long long ldl = (words_of(l) + 1) & ~1ll, wn = words_of(n), ldn = (wn + 1) & ~1ll, ldct = (passes + 1) & ~1ll;
      const size_t wBt = (size_t)n * ldl, wAt = (size_t)l * 2, wCt = (size_t)n * ldct, wTmp = accumulate ? (size_t)m * ldn : 0;
      void *ws = nullptr;
      if (gf2_stream_scratch(s, (wBt + wAt + wCt + wTmp) * sizeof(u64), &ws, GF2_SLOT_OPERANDS) == 0) {
        u64 *Bt = static_cast<u64 *>(ws), *At = Bt + wBt, *Ct = At + wAt, *Tmp = Ct + wCt;
        HIP_TRY(gf2k_transpose(Bt, ldl, B->data, B->ld, l, n, s));  // n x l
        for (int p = 0; p < passes; ++p) {
          const int mp = std::min(64, m - 64 * p);
          HIP_TRY(gf2k_transpose(At, 2, A->data + (long long)64 * p * A->ld, A->ld, mp, l, s));  // l x mp (one word per row)
          HIP_TRY(gf2k_tallskinny_long(Bt, ldl, At, 2, Ct + p, ldct, n, l, mp, 0, s));           // word p of the n rows of C^T
        }
        if (accumulate) {
          HIP_TRY(gf2k_transpose(Tmp, ldn, Ct, ldct, n, m, s));  // m x n
          HIP_TRY(gf2k_xor2d(C->data, C->ld, C->data, C->ld, Tmp, ldn, m, (int)wn, s));
        } else {
          HIP_TRY(gf2k_transpose(C->data, C->ld, Ct, ldct, n, m, s));
        }
        return 0;
      }
    }
  }
  // A tall product may first copy A into the row-group-packed layout (one extra pass over A, ~0.2 ms per GiB) so that the
  // paired tile kernels fetch it with contiguous loads: taken when the modelled launch gains more than the pass costs
  const long long wp = (words_of(l) + 1) & ~1ll, prow = ((long long)m + 63) & ~63ll;
  const PlainPlan pp = plain_plan(m, l, n);
  bool packed = pp.pack;
  TilePlan tp = pp.tp;
  const u64 *Aptr = A->data;
  long long lda = A->ld;
  if (packed) {
    void *pa = nullptr;
    if (gf2_stream_scratch(s, (size_t)(prow * wp * 8), &pa, GF2_SLOT_PACKED_A) == 0) {
      HIP_TRY(gf2k_packA(static_cast<u64 *>(pa), wp, A->data, A->ld, m, words_of(l), s));
      Aptr = static_cast<const u64 *>(pa);
      lda = wp;
    } else {
      packed = false;
      tp = plan_tiles(m, l, n, 1, false);
    }
  }
  // buffer descriptors of the tile kernel carry 32-bit byte counts: one tile of A rows must stay below 4 GiB
  if ((!packed && (long long)A->ld * 8 * 4096 >= (1ll << 32)) || (long long)B->ld * 8 * 32 >= (1ll << 31))
    return gf2_fail_msg("gf2_mul_dev: row stride too large for the tile kernel (more than ~8 million columns)");
  gf2k_mul_args a{};
  a.A = Aptr;
  a.a_packed = packed ? 1 : 0;
  a.B = B->data;
  a.C = C->data;
  a.lda = lda;
  a.ldb = B->ld;
  a.ldc = C->ld;
  a.m = m;
  a.l = l;
  a.n = n;
  a.batch = 1;
  a.accumulate = accumulate;
  return launch_planned(a, tp, s);
}

static constexpr int kSupp[2][7][2] = GF2_STRASSEN_SUPP;  // (gf2_variants.h: the split kernels read the same table)

static int mul_strassen(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, int L, hipStream_t s,
                        bool sync_free) {
  const int m = A->nrows, l = A->ncols, n = B->ncols;
  // the level passes use 16-byte accesses: row strides must be even and the bases 16-byte aligned
  if ((A->ld | B->ld | C->ld) & 1) L = 0;
  if ((reinterpret_cast<uintptr_t>(A->data) | reinterpret_cast<uintptr_t>(B->data) | reinterpret_cast<uintptr_t>(C->data)) & 15) L = 0;
  if (L <= 0) return gf2_mul_m4rm_plain(C, A, B, accumulate, s);
  if (L > 6) L = 6;
  const StrassenArena arena = strassen_arena(m, l, n, L);
  void *ws = nullptr;
  if (int rc = gf2_stream_scratch(s, arena.words * sizeof(u64), &ws, GF2_SLOT_OPERANDS)) return rc;
  const std::vector<PlanStep> plan = strassen_plan(L);
  u64 *Aop[7], *Bop[7], *Pop[7];  // operands and products of level i (of the levels the plan materialises)
  auto at = [&](size_t off) { return off == StrassenArena::none ? nullptr : static_cast<u64 *>(ws) + off; };
  for (int i = 0; i < 7; ++i) Aop[i] = at(arena.a[i]), Bop[i] = at(arena.b[i]), Pop[i] = at(arena.p[i]);
  // leaf operands of A in the row-group-packed layout of the paired tile kernel (its A loads become contiguous): written by
  // the last split pass when that pass is a fused one
  bool a_packed = false;
  const TilePlan leaf = leaf_plan(m, l, n, L, &a_packed);

  // one split step on one side: operands of level `prev` (7^prev of them, or the caller's matrix) -> level i
  auto split_step = [&](const PlanStep &st, int prev, int i, int side, bool pack) -> int {
    const bool isA = side == 0;
    const int rows_prev = (isA ? m : l) >> prev, rows_i = (isA ? m : l) >> i;
    const int words_prev = ((isA ? l : n) >> prev) / 64, words_i = ((isA ? l : n) >> i) / 64;
    const int batch = (int)pow7(prev);
    const gf2_dmat *top = isA ? A : B;
    const u64 *src = prev ? (isA ? Aop[prev] : Bop[prev]) : top->data;
    const long long lds_ = prev ? (long long)words_prev : top->ld;
    const long long srcStride = prev ? (long long)rows_prev * lds_ : 0;
    u64 *dst = isA ? Aop[i] : Bop[i];
    const long long dstStride = (long long)rows_i * words_i;
    const int kside = pack ? 2 : side;
    if (st.k == 1) return (int)gf2k_strassen_split(dst, words_i, dstStride, src, lds_, srcStride, rows_i, words_i, kside, batch, s);
    if (st.k == 2) return (int)gf2k_strassen_split2(dst, words_i, dstStride, src, lds_, srcStride, rows_i, words_i, kside, batch, s);
    const u64 *s0[7], *s1[7];
    int groups = 1;
    s0[0] = src;
    s1[0] = nullptr;
    if (st.virt) {
      groups = 7;
      const long long hq = rows_prev / 2, wq = words_prev / 2;  // quadrants of the source operand
      auto quad = [&](int q) { return src + (long long)(q >> 1) * hq * lds_ + (long long)(q & 1) * wq; };
      for (int g = 0; g < 7; ++g) {
        s0[g] = quad(kSupp[side][g][0]);
        s1[g] = kSupp[side][g][1] >= 0 ? quad(kSupp[side][g][1]) : nullptr;
      }
    }
    return (int)gf2k_strassen_split3(dst, words_i, dstStride, s0, s1, groups, lds_, srcStride, rows_i, words_i, kside, batch, s);
  };

  auto run = [&]() -> int {
    int prev = 0;
    for (size_t k = 0; k < plan.size(); ++k) {
      const int i = prev + plan[k].levels();
      const bool last = k + 1 == plan.size();
      HIP_TRY((hipError_t)split_step(plan[k], prev, i, 0, last && a_packed));
      HIP_TRY((hipError_t)split_step(plan[k], prev, i, 1, false));
      prev = i;
    }
    {  // all 7^L leaf products in one batched launch
      const int mL = m >> L, lL = l >> L, nL = n >> L;
      gf2k_mul_args a{};
      a.lda = lL / 64;
      a.ldb = nL / 64;
      a.ldc = nL / 64;
      a.sA = (long long)mL * a.lda;
      a.sB = (long long)lL * a.ldb;
      a.sC = (long long)mL * a.ldc;
      a.A = Aop[L];
      a.B = Bop[L];
      a.C = Pop[L];
      a.m = mL;
      a.l = lL;
      a.n = nL;
      a.batch = (int)pow7(L);
      a.accumulate = 0;
      a.a_packed = a_packed ? 1 : 0;
      if (int r = launch_planned(a, leaf, s)) return r;
    }
    // fold the products back up
    int i = L;
    for (int k = (int)plan.size() - 1; k >= 0; --k) {
      const PlanStep &st = plan[k];
      const int up = i - st.levels();  // products of level i -> level `up`
      const int mi = m >> i, wi = (n >> i) / 64, batch = (int)pow7(up);
      u64 *dst = up ? Pop[up] : C->data;
      const long long ldd = up ? (long long)((n >> up) / 64) : C->ld;
      const long long strD = up ? (long long)(m >> up) * ldd : 0;
      const int acc = up ? 0 : accumulate;
      const long long dP = (long long)mi * wi;
      if (st.k == 1) {
        HIP_TRY(gf2k_strassen_merge(dst, ldd, strD, Pop[i], wi, dP, mi, wi, acc, batch, s));
      } else if (st.k == 2) {
        HIP_TRY(gf2k_strassen_merge2(dst, ldd, strD, Pop[i], wi, dP, mi, wi, acc, batch, s));
      } else if (!st.virt) {
        HIP_TRY(gf2k_strassen_merge3(dst, ldd, strD, Pop[i], wi, dP, mi, wi, acc, 1, batch, s));
      } else {
        // the 7 parents of the virtual level are never written: their sums live in LDS (the arena's slots for them go unused)
        HIP_TRY(gf2k_strassen_merge4(dst, ldd, strD, Pop[i], wi, dP, mi, wi, acc, batch, s));
      }
      i = up;
    }
    return 0;
  };
  const int rc = run();
  return rc ? rc : sync_if(sync_free, s);
}

// The operand arena of L levels must fit what the stream's arena may grow to (gf2_dev_arena_limit).
// `extra_bytes`: what the caller allocates besides the arena (the zero-padded copies of a padded product).
static int cap_levels_by_memory(int m, int l, int n, int L, hipStream_t s, size_t extra_bytes = 0) {
  if (L <= 0) return L;
  const size_t avail = gf2_dev_arena_limit(s);
  while (L > 0 && strassen_arena(m, l, n, L).words * sizeof(u64) + extra_bytes > avail) --L;
  return L;
}

std::mutex gf2_enqueue_mu;

static int mul_strassen_padded(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, const MulPlan &pp, hipStream_t s) {
  const int m = A->nrows, l = A->ncols, n = B->ncols;
  const int mp = pp.d[0], lp = pp.d[1], np = pp.d[2];  // the padded dimensions
  const long long wa = lp / 64, wb = np / 64;
  const size_t wordsA = (size_t)mp * wa, wordsB = (size_t)lp * wb, wordsC = (size_t)mp * wb;
  void *ws = nullptr;
  if (int rc = gf2_stream_scratch(s, (wordsA + wordsB + wordsC) * sizeof(u64), &ws, GF2_SLOT_PADDED)) return rc;
  u64 *pa = static_cast<u64 *>(ws), *pb = pa + wordsA, *pc = pb + wordsB;
  HIP_TRY(gf2k_padcopy(pa, wa, mp, (int)wa, A->data, A->ld, m, l, s));
  HIP_TRY(gf2k_padcopy(pb, wb, lp, (int)wb, B->data, B->ld, l, n, s));
  gf2_dmat Ap{pa, wa, mp, lp}, Bp{pb, wb, lp, np}, Cp{pc, wb, mp, np};
  if (int rc = mul_strassen(&Cp, &Ap, &Bp, 0, pp.L, s, false)) return rc;
  // rows / columns past the operands are zero in the padded product, so whole words of the corner are exact
  HIP_TRY(gf2k_xor2d(C->data, C->ld, pc, wb, accumulate ? C->data : nullptr, C->ld, m, words_of(n), s));
  return 0;
}

// core through Strassen in place (views of the caller's buffers: the core's column offsets are multiples of 128 bits), borders plain
static int mul_strassen_peeled(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, const MulPlan &pp, hipStream_t s) {
  const int m = A->nrows, l = A->ncols, n = B->ncols;
  const int mc = pp.d[0], lc = pp.d[1], nc = pp.d[2];
  gf2_dmat Ac{A->data, A->ld, mc, lc}, Bc{B->data, B->ld, lc, nc}, Cc{C->data, C->ld, mc, nc};
  if (int rc = mul_strassen(&Cc, &Ac, &Bc, accumulate, pp.L, s, false)) return rc;
  // a border strip: the level count among those that divide it (no further padding / peeling), capped by memory
  auto strip = [&](gf2_dmat *Cs, const gf2_dmat *As, const gf2_dmat *Bs, int acc) -> int {
    int Ls = pick_levels(As->nrows, As->ncols, Bs->ncols, 0, strassen_leaf_min());
    Ls = cap_levels_by_memory(As->nrows, As->ncols, Bs->ncols, Ls, s);
    return mul_strassen(Cs, As, Bs, acc, Ls, s, false);
  };
  if (l > lc) {  // tail of the inner dimension: core block of C ^= A[0:mc, lc:l] * B[lc:l, 0:nc]
    gf2_dmat At{A->data + lc / 64, A->ld, mc, l - lc}, Bt{B->data + (long long)lc * B->ld, B->ld, l - lc, nc};
    if (int rc = strip(&Cc, &At, &Bt, 1)) return rc;
  }
  if (n > nc) {  // right columns
    gf2_dmat Ar{A->data, A->ld, mc, l}, Br{B->data + nc / 64, B->ld, l, n - nc}, Cr{C->data + nc / 64, C->ld, mc, n - nc};
    if (int rc = strip(&Cr, &Ar, &Br, accumulate)) return rc;
  }
  if (m > mc) {  // bottom rows
    gf2_dmat Ab{A->data + (long long)mc * A->ld, A->ld, m - mc, l}, Cb{C->data + (long long)mc * C->ld, C->ld, m - mc, n};
    if (int rc = strip(&Cb, &Ab, B, accumulate)) return rc;
  }
  return 0;
}

static int mul_naive_dev(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, hipStream_t s,
                         bool sync_free) {
  // mzd_mul_naive (mzd.rs:150-152) = transpose B, then the row-parity product (mzd.rs:154-168).
  // For wide B the table kernel computes the same bits far faster, so only narrow products
  // (C one word wide: the matrix x vector path of mul_slice, binary_matrix.rs:416-431) take this route.
  const int m = A->nrows, l = A->ncols, n = B->ncols;
  if (n > 64 || l == 0) return gf2_mul_m4rm_plain(C, A, B, accumulate, s);
  if (m == 0 || n == 0) return 0;
  if (ts_long_shape(m, l, n)) {
    HIP_TRY(gf2k_tallskinny_long(A->data, A->ld, B->data, B->ld, C->data, C->ld, m, l, n, accumulate, s));
    return sync_if(sync_free, s);
  }
  if (widevec_shape(m, l, n)) {  // long rows: a wave per row
    if (int rc = mul_widevec(C, A, B, accumulate, s)) return rc;
    return sync_if(sync_free, s);
  }
  if (n > 8 && m >= 2048) return gf2_mul_m4rm_plain(C, A, B, accumulate, s);  // batch of vectors: table kernel (see there)
  // one to eight vectors against MANY short rows (`&A * &v` on 2^20 LPN samples): the 8-bit table kernel of gf2_lpn.inc streams A
  // with wave-contiguous non-temporal loads and costs the same whatever n <= 64 is (2^20 x 256 x 1 cold: 9.4 us through the
  // AND / popcount kernel below, 8.7-8.9 through the tables); with fewer rows the popcount kernel's small workgroups start faster
  static const int narrow_lpn_rows = dev_env_int("M4RI_HIP_NARROW_LPN_ROWS", 262144);
  if (narrow_lpn_rows > 0 && m >= narrow_lpn_rows && l <= 256 && l > 64) {
    HIP_TRY(gf2k_tallskinny(A->data, A->ld, B->data, B->ld, C->data, C->ld, m, l, n, accumulate, s));
    return sync_if(sync_free, s);
  }
  if ((size_t)n * words_of(l) * 8 <= 65536) {  // one launch: B is transposed into LDS by every block
    hipError_t e1 = gf2k_narrow(A->data, A->ld, B->data, B->ld, C->data, C->ld, m, l, n, accumulate, s);
    if (e1 != hipSuccess) return gf2_fail_hip(e1, "gf2k_narrow");
    return sync_if(sync_free, s);
  }
  const long long ldbt = (words_of(l) + 1) & ~1ll;
  const size_t bytes = (size_t)n * ldbt * sizeof(u64);
  void *bt = nullptr;
  if (int rc = gf2_stream_scratch(s, bytes, &bt, GF2_SLOT_OPERANDS)) return rc;
  hipError_t e = gf2k_transpose(static_cast<u64 *>(bt), ldbt, B->data, B->ld, l, n, s);
  if (e != hipSuccess) return gf2_fail_hip(e, "gf2k_transpose");
  e = gf2k_rowparity(A->data, A->ld, static_cast<u64 *>(bt), ldbt, C->data, C->ld, m, l, n, accumulate, s);
  if (e != hipSuccess) return gf2_fail_hip(e, "gf2k_rowparity");
  return sync_if(sync_free, s);
}

// The argument and aliasing rules of gf2_mul_dev and gf2_mul_nt_dev (include/m4ri_hip.h), checked before a device is required.  A is
// m x l; B is l x n (nt: n x l); C is m x n.  A and B are only read and may be one matrix or overlap; C is written while other
// workgroups still read rows of A and B, so it may share no word with either.  0: go ahead; 1: C is empty, nothing to do; -1: refused
static int check_mul(const char *fn, const char *bname, const gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, bool nt) {
  if (gf2_check_mat(fn, "C", C) || gf2_check_mat(fn, "A", A) || gf2_check_mat(fn, bname, B)) return -1;
  if (A->ncols != (nt ? B->ncols : B->nrows) || C->nrows != A->nrows || C->ncols != (nt ? B->nrows : B->ncols))
    return gf2_bad_arg(fn, "dimension mismatch");
  if (C->nrows == 0 || C->ncols == 0) return 1;
  if (gf2_refuse_overlap(fn, "C", C, "A", A) || gf2_refuse_overlap(fn, "C", C, bname, B)) return -1;
  return 0;
}

// an inner dimension of 0: the product is the zero matrix
static int mul_of_nothing(const char *fn, gf2_dmat *C, int accumulate, hipStream_t s) {
  if (accumulate) return 0;
  return gf2_hip_rc(gf2k_xor2d(C->data, C->ld, nullptr, 0, nullptr, 0, C->nrows, words_of(C->ncols), s), fn);
}

int gf2_mul_dispatch(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, int algo, int param, hipStream_t s, bool sync_free) {
  std::unique_lock<std::mutex> lk(gf2_enqueue_mu, std::defer_lock);
  if (!sync_free) lk.lock();  // host-path calls own a private (thread-local) stream
  switch (algo) {
    case GF2_ALGO_NAIVE:
      return mul_naive_dev(C, A, B, accumulate, s, sync_free);
    case GF2_ALGO_M4RM: {
      const int rc = gf2_mul_m4rm_plain(C, A, B, accumulate, s);
      return rc ? rc : sync_if(sync_free, s);
    }
    case GF2_ALGO_AUTO:
    case GF2_ALGO_STRASSEN: {
      const int m = A->nrows, l = A->ncols, n = B->ncols;
      const MulPlan mp = plan_product(m, l, n, param, ((A->ld | B->ld | C->ld) & 1) == 0);
      if (mp.kind) {
        const size_t mp_ = mp.d[0], lp_ = mp.d[1], np_ = mp.d[2];
        // a padded product also holds the three padded copies (slot 3) next to the arena
        const size_t pad_bytes = mp.kind == 1 ? (mp_ * (lp_ / 64) + lp_ * (np_ / 64) + mp_ * (np_ / 64)) * sizeof(u64) : 0;
        if (cap_levels_by_memory(mp.d[0], mp.d[1], mp.d[2], mp.L, s, pad_bytes) == mp.L) {
          const int rc = mp.kind == 1 ? mul_strassen_padded(C, A, B, accumulate, mp, s) : mul_strassen_peeled(C, A, B, accumulate, mp, s);
          return rc ? rc : sync_if(sync_free, s);
        }
      }
      return mul_strassen(C, A, B, accumulate, cap_levels_by_memory(m, l, n, mp.L_given, s), s, sync_free);
    }
    default:
      return gf2_fail_msg("gf2_mul_dev: unknown algorithm");
  }
}

extern "C" int gf2_mul_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, int accumulate, int algo, int param,
                           void *stream) {
  static const char fn[] = "gf2_mul_dev";
  if (int rc = check_mul(fn, "B", C, A, B, false)) return rc < 0 ? rc : 0;
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (A->ncols == 0) return mul_of_nothing(fn, C, accumulate, s);
  return gf2_mul_dispatch(C, A, B, accumulate, algo, param, s, /*sync_free=*/false);
}

extern "C" int gf2_mul_nt_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *Bt, int accumulate, void *stream) {
  static const char fn[] = "gf2_mul_nt_dev";
  if (int rc = check_mul(fn, "Bt", C, A, Bt, true)) return rc < 0 ? rc : 0;
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int m = A->nrows, l = A->ncols, n = Bt->nrows;
  if (l == 0) return mul_of_nothing(fn, C, accumulate, s);
  if (widevec_shape(m, l, n)) {  // long rows, at most 64 vectors: a wave per row (Bt is already what that kernel reads)
    HIP_TRY(gf2k_widevec(A->data, A->ld, Bt->data, Bt->ld, C->data, C->ld, m, l, n < 32 ? n : 32, accumulate, 0, s));
    if (n > 32) HIP_TRY(gf2k_widevec(A->data, A->ld, Bt->data + 32 * Bt->ld, Bt->ld, C->data, C->ld, m, l, n - 32, 1, 32, s));
    return 0;
  }
  HIP_TRY(gf2k_rowparity(A->data, A->ld, Bt->data, Bt->ld, C->data, C->ld, m, l, n, accumulate, s));
  return 0;
}

extern "C" int gf2_strassen_levels(int m, int l, int n, int algo, int param) {
  if (algo != GF2_ALGO_AUTO && algo != GF2_ALGO_STRASSEN) return 0;
  int L = pick_levels(m, l, n, param, strassen_leaf_min());  // the planner's answer; with a device, capped by its memory
  int ndev = 0;
  if (L > 0 && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) L = cap_levels_by_memory(m, l, n, L, nullptr);
  else (void)hipGetLastError();
  return L;
}

// C = A xor B.  Every word is read and written by the one thread that owns it, so C may be A, B or both (mzd_add(A, A, B), the
// reference's +=); any other overlap of C with an operand would read words another thread has already replaced.
extern "C" int gf2_add_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream) {
  static const char fn[] = "gf2_add_dev";
  if (gf2_check_mat(fn, "C", C) || gf2_check_mat(fn, "A", A) || gf2_check_mat(fn, "B", B)) return -1;
  if (A->nrows != B->nrows || A->ncols != B->ncols || C->nrows != A->nrows || C->ncols != A->ncols)
    return gf2_bad_arg(fn, "dimension mismatch");
  if (C->nrows == 0 || C->ncols == 0) return 0;
  if (!gf2_same_view(C, A) && gf2_refuse_overlap(fn, "C", C, "A", A)) return -1;
  if (!gf2_same_view(C, B) && gf2_refuse_overlap(fn, "C", C, "B", B)) return -1;
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(gf2k_xor2d(C->data, C->ld, A->data, A->ld, B->data, B->ld, A->nrows, words_of(A->ncols), s));
  return 0;
}

extern "C" int gf2_transpose_dev(gf2_dmat *D, gf2_dmat const *S, void *stream) {
  static const char fn[] = "gf2_transpose_dev";
  if (gf2_check_mat(fn, "D", D) || gf2_check_mat(fn, "S", S)) return -1;
  if (D->nrows != S->ncols || D->ncols != S->nrows) return gf2_bad_arg(fn, "dimension mismatch");
  if (S->nrows == 0 || S->ncols == 0) return 0;
  if (gf2_refuse_overlap(fn, "D", D, "S", S)) return -1;
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(gf2k_transpose(D->data, D->ld, S->data, S->ld, S->nrows, S->ncols, s));
  return 0;
}

// both matrices are only read: they may be one matrix or overlap in any way
extern "C" int gf2_equal_dev(gf2_dmat const *A, gf2_dmat const *B, int *equal, void *stream) {
  static const char fn[] = "gf2_equal_dev";
  if (gf2_check_mat(fn, "A", A) || gf2_check_mat(fn, "B", B)) return -1;
  GF2_RC(gf2_refuse_null(fn, "equal", equal));
  if (A->nrows != B->nrows || A->ncols != B->ncols) {
    *equal = 0;
    return 0;
  }
  if (A->nrows == 0 || A->ncols == 0) {
    *equal = 1;
    return 0;
  }
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  void *flag = nullptr;
  if (int rc = gf2_dev_alloc(&flag, sizeof(int))) return rc;
  int host = 0, rc = 0;
  do {
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e == hipSuccess) e = gf2k_diff(A->data, A->ld, B->data, B->ld, A->nrows, A->ncols, static_cast<int *>(flag), s);
    if (e == hipSuccess) e = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = gf2_fail_hip(e, "gf2_equal_dev");
  } while (0);
  gf2_dev_free(flag, sizeof(int));
  *equal = host ? 0 : 1;
  return rc;
}

