// mul_plan_host.cpp -- the launch planner: tile plans, Strassen level plans, pad / peel shape plans and the schedules of a host
// product, chosen by modelled time; and the exported queries that report them.  No HIP: everything here runs without a device.
#include <array>
#include <cmath>
#include <cstdio>
#include <unordered_map>

#include "../../include/m4ri_hip.h"
#include "mul_plan.h"

typedef uint64_t u64;

int strassen_leaf_min() {
  static const int leaf_min = env_int("M4RI_HIP_STRASSEN_LEAF_MIN", 2048);
  return leaf_min;
}

// ---- launch geometry of the tile kernel (shared by the launcher and the level chooser) ----
// tile geometry and measured cost of the OLDER kernel variants (gf2_kernels.hip): 8 = v6 2048 x 1024 tile, two chunks per lookup step, one
// row per lane; 7 = v3 1024 x 2048 tile; 20 = v3 256 x 2048 tile (4 waves).  (The v8 family, 9-12, is priced by v8_model below;
// 90-99 are the legacy v7 of development builds.)  M4RI_HIP_M4RM_CFG overrides (shipped variants only)
struct TileGeom {
  int rows, cols;
  double cyc_per_chunk;  // measured cycles per 8 bits of the inner dimension and tile, 2.4 GHz
};
static TileGeom tile_geom(int cfg, bool packed = false) {
  const gf2_variant v = gf2_variant_of(cfg);  // the geometry is the launcher's; the cost is per family (v7, v6, v3 with 4 waves, v3)
  return {v.rows, v.cols, v.cols == 512 ? (packed ? 1520.0 : 1800.0) : v.cols == 1024 ? (packed ? 1620.0 : 1790.0) : v.rows == 256 ? 1300.0 : 2350.0};
}
static long long tiles_of(const TileGeom &g, int m, int n) {
  return (long long)((m + g.rows - 1) / g.rows) * ((n + g.cols - 1) / g.cols);
}

static bool cfg_reads_packed(int cfg) { return gf2_variant_of(cfg).reads_packed; }
static int cfg_v8_rg(int cfg) { return gf2_variant_of(cfg).v8_rg; }

// split-K factor of the older kernels (v3, v6): when a product has too few tiles to fill 256 CUs, the inner dimension is cut into
// slices of at least 128 bits; the slices' partial products are combined by a second kernel
static int m4rm_ksplit_for(int m, int l, int n, int batch, int cfg) {
  static const int forced = dev_env_int("M4RI_HIP_M4RM_KSPLIT", 0);
  if (forced > 0) return forced;
  const long long wg = tiles_of(tile_geom(cfg), m, n) * batch;
  const int nw32 = (l + 31) / 32;
  if (wg >= 192) {
    // All tiles of a launch take the same time, so 520 workgroups cost three rounds of 256 where 2.03 would do.  A single plain
    // product may cut the inner dimension into a few slices to even the rounds out (the slices' partial tiles cost one write and
    // one read of C per slice): rounds(ks) / ks tile-times + ks passes over C, minimised over ks <= 8.
    static const int balance = dev_env_int("M4RI_HIP_SPLITK_BALANCE", 1);
    static const long long cap = (long long)env_int("M4RI_HIP_SPLITK_WS_MIB", 2048) << 20;
    if (!balance || batch != 1 || wg > 2048) return 1;
    const TileGeom g = tile_geom(cfg, cfg == 8);
    const double tile_cyc = (double)nw32 * 4.0 * g.cyc_per_chunk;                       // one whole-k tile
    const double pass_cyc = 2.0 * (double)m * (double)n / 8.0 / 5.0e12 * 2.4e9;         // write + read of one slice's partial C
    int best = 1;
    double best_c = std::ceil(wg / 256.0) * (tile_cyc + 20000.0);
    for (int ks = 2; ks <= 8; ++ks) {
      if (nw32 / ks < 16) break;                                                        // slices of at least 512 bits
      if ((long long)ks * m * ((words_of(n) + 1) & ~1) * 8 > cap) break;
      const double c = std::ceil(wg * ks / 256.0) * (tile_cyc / ks + 20000.0) + ks * pass_cyc;
      if (c < 0.93 * best_c) best = ks, best_c = c;
    }
    return best;
  }
  long long ks = 256 / wg;  // one round of workgroups: 256 long slices beat 512 short ones (8192x65536x16384: 2.25 vs 2.52 ms)
  if (ks > nw32 / 4) ks = nw32 / 4;  // slices of at least 128 bits
  return ks < 1 ? 1 : (int)ks;
}

// ---- which tile kernel, and how its launch is cut (shared by the launchers and the level chooser) ----
// Candidates: the v8 family (512 RG rows x 512 columns, RG = 8 / 4 / 2 / 1: variants 9 / 10 / 11 / 12) with whole tiles, or with
// the tiles of the last (incomplete) round of 256 workgroups cut into stream-K segments (everything, when there are fewer than
// 256 tiles); v6 (8) and v3 (7, and 20 for m <= 256) with their uniform split-K.  Chosen by modelled time; the constants are
// measured (tools/kbench, profiles/r03_tile_variants.txt).  `packed`: A is handed over row-group packed (Strassen leaves, or a
// plain product that packs A itself): only 8 and 9-12 read that layout.
// microseconds per quad (32 bits of the inner dimension) of a v8 tile: table generation (256 entry writes, barrier) + RG x 1024
// lookups; an unpacked A costs 64 scattered 8-byte loads per wave and row group.  Measured on 343 leaves of 4096^3
// (profiles/r03_tile_variants.txt): packed 0.71 / 0.96 / 1.46 / 2.55 us per quad and tile for RG = 1 / 2 / 4 / 8 INCLUDING the
// tile's prologue / epilogue / hand-over, which v8_model adds separately ((3.4 + 0.6 RG) us per 128 quads there): the loop
// itself takes 0.679 / 0.924 / 1.415 / 2.486 us (M4RI_HIP_V8_QUAD_NS overrides the four; checked against 49 leaves of
// 5632^3 in 2048-row tiles: 1617 tiles x 176 quads in 1.63 ms = 1.47 us per quad and tile all in)
// Unpacked A with LONG rows: a lane's 8-byte loads walk its own row, and from ~8192 bits on the lines the 4096 rows of a
// tile keep open (64 bytes each) no longer survive in L2 until their next word is wanted -- every load fetches a line from
// HBM (65536 x 65536 x 512: 1.14 ms unpacked, 0.78 ms with the packing pass; 65536 x 8192 x 512: 0.190 against 0.101 ms;
// up to 7000 bits packing loses, 0.092 against 0.156 ms): the surcharge is five times as high from 8192 bits on.
static double v8_quad_us(int RG, bool packed, int l = 0) {
  static const double unp0 = dev_env_int("M4RI_HIP_V8_UNPACKED_BASE_NS", 100) * 1e-3, unp = dev_env_int("M4RI_HIP_V8_UNPACKED_NS", 70) * 1e-3;
  static const std::array<double, 4> loop_us = [] {
    std::array<double, 4> t{0.679, 0.924, 1.415, 2.486};
#ifdef GF2K_DEV_VARIANTS  // (M4RI_HIP_V8_QUAD_NS=a,b,c,d: the loop's nanoseconds per quad at 512 / 1024 / 2048 / 4096 rows, for model fits)
    if (const char *e = getenv("M4RI_HIP_V8_QUAD_NS")) {
      int v[4];
      if (std::sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]) == 4)
        for (int i = 0; i < 4; ++i) t[i] = v[i] * 1e-3;
    }
#endif
    return t;
  }();
  const int i = RG >= 8 ? 3 : RG >= 4 ? 2 : RG >= 2 ? 1 : 0;
  static const double long_rows = dev_env_int("M4RI_HIP_V8_UNPACKED_LONG_PCT", 500) * 1e-2;
  const double stretch = l >= 8192 ? long_rows : 1.0;  // a cliff, not a slope: 65536 x l x 512 unpacked takes 0.092 ms at l = 7000 and 0.188 ms at 8192
  return loop_us[i] + (packed ? 0.0 : (unp0 + unp * RG) * stretch);
}

// One v8 launch: `batch` products, variant cfg, the last n_rem tiles cut into about `want` segments (n_rem = 0: whole tiles only).
// Fills c (the cut is gf2_streamk_cut_of's, which the launcher applies too) and returns false if the cut is void or its
// scratch exceeds the cap.
static bool v8_model(int m, int l, int n, int batch, bool packed, int cfg, long long n_rem, long long want, TilePlan &c) {
  static const long long cap = (long long)env_int("M4RI_HIP_SPLITK_WS_MIB", 2048) << 20;
  static const double seg_fix = dev_env_int("M4RI_HIP_V8_SEG_FIX_NS", 3500) * 1e-9, seg_rg = dev_env_int("M4RI_HIP_V8_SEG_RG_NS", 2600) * 1e-9,
                      red_bw = dev_env_int("M4RI_HIP_V8_REDUCE_GBS", 2500) * 1e9, two_part = dev_env_int("M4RI_HIP_V8_TWO_PART_PCT", 180) * 1e-2;
  const int RG = cfg_v8_rg(cfg), R = 512 * RG, nw32 = (l + 31) / 32, Q = (nw32 + 1) / 2;
  const long long T = (long long)((m + R - 1) / R) * ((n + 511) / 512) * batch;
  const double tq = v8_quad_us(RG, packed, l) * 1e-6, tile_bytes = R * 64.0;
  const double tile_t = 2.0 * Q * tq + (3.4 + 0.6 * RG) * 1e-6;  // + prologue, epilogue (LDS transpose, stores), hand-over to the next workgroup
  c = TilePlan();
  c.cfg = cfg;
  c.packed = packed;
  if (n_rem <= 0 || Q < 1) {
    c.t = std::ceil(T / 256.0) * tile_t + 2e-6;
    return true;
  }
  const gf2_streamk_cut cut = gf2_streamk_cut_of(T, Q, n_rem, want);
  if (cut.n_rem == 0) return false;  // nothing is cut
  n_rem = cut.n_rem;
  const long long ns = cut.nseg, seg = cut.seg;
  c.n_rem = (int)n_rem;
  c.nseg = (int)ns;
  c.ws_bytes = (size_t)gf2_streamk_words(gf2_variant_of(cfg), ns) * sizeof(u64);
  if ((long long)c.ws_bytes > cap || ns > (1 << 22)) return false;
  // partial tiles: written at the end of the segment phase (every workgroup at once: ~2.6 us per row group on top of the
  // prologue; a segment that spans two tiles pays prologue and stores twice), read back and folded into C by the reduction
  // kernel (launch gap + bytes at ~2.5 TB/s)
  const bool spans = (Q % seg) != 0;
  const double slots = (double)ns + (spans ? (double)std::min(ns, n_rem) : 0.0);
  const double reduce_t = (slots + (double)n_rem) * tile_bytes / red_bw + 2.5e-6;
  const double seg_t = 2.0 * seg * tq + (seg_fix + seg_rg * RG) * (spans ? two_part : 1.0);
  c.t = std::ceil((T - n_rem) / 256.0) * tile_t + std::ceil(ns / 256.0) * seg_t + reduce_t + 2e-6;
  return true;
}

static bool older_model(int m, int l, int n, int batch, bool packed, int cfg, TilePlan &c) {
  static const long long cap = (long long)env_int("M4RI_HIP_SPLITK_WS_MIB", 2048) << 20;
  if (packed && !cfg_reads_packed(cfg)) return false;
  const int nw32 = (l + 31) / 32;
  const TileGeom g = tile_geom(cfg, packed);
  const int ks = m4rm_ksplit_for(m, l, n, batch, cfg);
  const double wg = (double)tiles_of(g, m, n) * batch * ks;
  const double chunks = std::ceil(nw32 / (double)ks) * 4.0;
  c = TilePlan();
  c.cfg = cfg;
  c.ksplit = ks;
  c.packed = packed;
  c.t = std::ceil(wg / 256.0) * (chunks * g.cyc_per_chunk + 6000.0) / 2.4e9 + 3e-6;
  // measured against the v8 plans on narrow products with long rows (2048 x 33000 x 600: modelled 44 us, 83 measured with 256
  // slices; 9000 x 33000 x 300: 82 / 127 with 51; 33000 x 9000 x 300: 77 / 111 with 15; the same shapes through v8 on packed A:
  // 39-74 us): unpacked rows of 8192 bits and more cost these kernels 1.4x (they too read a row per lane or lane group), and
  // every slice of the inner dimension another 0.2 %
  static const double older_long = dev_env_int("M4RI_HIP_OLDER_LONG_PCT", 140) * 1e-2, older_ks = dev_env_int("M4RI_HIP_OLDER_KSPLIT_PPM", 2000) * 1e-6;
  if (!packed && l >= 8192) c.t *= older_long;
  c.t *= 1.0 + older_ks * ks;
  if (ks > 1) {
    const double part = (double)m * (double)(((words_of(n) + 1) & ~1) * 8) * batch;
    c.ws_bytes = (size_t)(part * ks);
    c.t += (part * ks * 2.0 + part) / 4.0e12 + 2.5e-6;
    if ((long long)c.ws_bytes > cap) return false;
  }
  return true;
}

static TilePlan plan_tiles_uncached(int m, int l, int n, int batch, bool packed, int mode);
// Planning is pure arithmetic on the shape (and the environment, read once), but a level choice evaluates dozens of candidate
// launches: 15-55 us of host time per product, which a 0.2 ms product notices.  Every thread keeps what it has planned.
struct PlanKey {
  int m, l, n, batch, flags;
  bool operator==(const PlanKey &o) const { return m == o.m && l == o.l && n == o.n && batch == o.batch && flags == o.flags; }
};
struct PlanKeyHash {
  size_t operator()(const PlanKey &k) const {
    size_t h = (size_t)k.m * 0x9E3779B97F4A7C15ull;
    h ^= ((size_t)k.l + 0x7F4A7C15u) * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
    h ^= ((size_t)k.n + 0x165667B1u) * 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h ^= ((size_t)k.batch * 31 + (size_t)k.flags) * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
    return h;
  }
};
template <class V, class F>
static V memoised(std::unordered_map<PlanKey, V, PlanKeyHash> &memo, const PlanKey &key, F compute) {
  auto it = memo.find(key);
  if (it != memo.end()) return it->second;
  if (memo.size() > 8192) memo.clear();
  const V v = compute();  // (may plan sub-shapes through the same memo)
  memo.emplace(key, v);
  return v;
}
TilePlan plan_tiles(int m, int l, int n, int batch, bool packed, int mode) {
  thread_local std::unordered_map<PlanKey, TilePlan, PlanKeyHash> memo;
  return memoised(memo, PlanKey{m, l, n, batch, (packed ? 1 : 0) | mode}, [&] { return plan_tiles_uncached(m, l, n, batch, packed, mode); });
}

static TilePlan plan_tiles_uncached(int m, int l, int n, int batch, bool packed, int mode) {
  const bool allow_tail = (mode & PLAN_TAIL) != 0;
  // A/B override, restricted to variants that compute the product (the timing-only ablations exist only in development
  // builds of the kernels and would be hipErrorInvalidValue here anyway)
  static const int forced = [] {
    const int f = env_int("M4RI_HIP_M4RM_CFG", -1);
#ifdef GF2K_DEV_VARIANTS
    return f;
#else
    if (f < 0 || gf2_variant_of(f).shipped) return f;
    std::fprintf(stderr, "m4ri_hip: M4RI_HIP_M4RM_CFG=%d ignored (accepted: 7, 8, 9, 10, 11, 12, 20, 81, 82)\n", f);
    return -1;
#endif
  }();
  static const int forced_ks = dev_env_int("M4RI_HIP_M4RM_KSPLIT", 0);
  static const int streamk = dev_env_int("M4RI_HIP_STREAMK", 1);      // 0: whole tiles only
  static const int tails = dev_env_int("M4RI_HIP_TAIL_LAUNCH", 1);    // 0: never cut a batched launch in two
  TilePlan best, c;
  bool have = false;
  auto consider = [&](const TilePlan &x) {
    if (!have || x.t < best.t) best = x, have = true;
  };
  auto v8 = [&](int cfg) {
    const int R = 512 * cfg_v8_rg(cfg);
    const long long tp = (long long)((m + R - 1) / R) * ((n + 511) / 512), T = tp * batch;
    if (forced_ks > 0) {
      if (v8_model(m, l, n, batch, packed, cfg, T, T * forced_ks, c) || v8_model(m, l, n, batch, packed, cfg, 0, 0, c)) consider(c);
      return;
    }
    if (v8_model(m, l, n, batch, packed, cfg, 0, 0, c)) consider(c);
    if (T < 1) return;
    const long long rem = T < 256 ? T : T % 256;
    if (rem == 0) return;
    if (streamk && v8_model(m, l, n, batch, packed, cfg, rem, 256, c)) consider(c);
    // the last products in a launch of their own: the first launch keeps whole rounds of 256 tiles
    if (tails && allow_tail && forced < 0 && batch > 1 && T > 256) {
      const long long b1 = (T - rem) / tp;  // products whose tiles all lie in the whole rounds
      if (b1 >= 1 && b1 < batch) {
        TilePlan head;
        if (v8_model(m, l, n, (int)b1, packed, cfg, 0, 0, head)) {
          const TilePlan tail = plan_tiles(m, l, n, batch - (int)b1, packed, 0);
          head.t += tail.t + 1.5e-6;
          head.tail_batch = batch - (int)b1;
          head.tail = {tail.cfg, tail.n_rem, tail.nseg, tail.ws_bytes};
          if (cfg_v8_rg(tail.cfg)) consider(head);
        }
      }
    }
  };
  if (forced >= 0) {
    if (cfg_v8_rg(forced)) v8(forced);
    else if (older_model(m, l, n, batch, packed, forced, c)) consider(c);
    if (!have) {  // a forced variant that cannot read this operand layout (the caller asks again unpacked), or whose split-K scratch
      // exceeds M4RI_HIP_SPLITK_WS_MIB: the plan carries no scratch, so the launcher runs it unsplit, and the query says so.  (`packed`
      // is cleared in both cases, on purpose: the callers decide the layout by the variant -- cfg_reads_packed -- not by this field)
      best.cfg = forced;
      best.packed = false;
      best.ksplit = 1;
      TilePlan est;  // (its time: the estimate of whole 512-row tiles, so that the level / shape planners never see a free launch)
      if (v8_model(m, l, n, batch, false, 12, 0, 0, est)) best.t = est.t;
    }
    return best;
  }
  const bool v8_only = (mode & PLAN_V8_ONLY) != 0;
  if (m <= 256 && !packed && !v8_only) {
    if (older_model(m, l, n, batch, packed, 20, c)) consider(c);
    if (have) return best;  // (rejected only when its split-K scratch exceeds M4RI_HIP_SPLITK_WS_MIB: the general candidates follow)
  }
  if (!v8_only) {
    if (!packed && older_model(m, l, n, batch, packed, 7, c)) consider(c);
    if (older_model(m, l, n, batch, packed, 8, c)) consider(c);
  }
  for (int cfg = 9; cfg <= 12; ++cfg) v8(cfg);
  // a row band: whole tile rows of 4096 (2048) in the main launch, the rows below them in a launch of their own with the
  // tile height that suits them (the same B, disjoint rows of A and C; the band's partial tiles reuse the scratch)
  static const int bands = dev_env_int("M4RI_HIP_ROW_BANDS", 1);
  static const double band_gain = dev_env_int("M4RI_HIP_ROW_BAND_MIN_GAIN_PCT", 3) * 1e-2;
  if (bands && (mode & PLAN_BAND) && have) {
    const TilePlan uniform = best;
    for (int R = 4096; R >= 2048; R >>= 1) {
      const int m1 = m / R * R, m2 = m - m1;
      if (m1 < R || m2 <= 0) continue;
      TilePlan head = plan_tiles(m1, l, n, batch, packed, (mode & PLAN_TAIL) | PLAN_V8_ONLY);
      const TilePlan band = plan_tiles(m2, l, n, batch, packed, PLAN_V8_ONLY);
      if (!cfg_v8_rg(head.cfg) || !cfg_v8_rg(band.cfg)) continue;
      // + the launch boundary between the two; batched leaves: priced 3 % up (measured at 40000^3 and 52000^3, where padded plans
      // with banded leaves were modelled 0.5 % ahead of the peeled plans and ran 3 % behind them; plain products match the model:
      // 17000^3 -9 %, 12700 x 1024 x 40000 -26 %, 70000^3's bottom strip 40.4 -> 39.1 ms)
      head.t = (head.t + band.t) * (batch > 1 ? 1.03 : 1.0) + 3e-6;
      if (head.t >= uniform.t * (1.0 - band_gain)) continue;
      head.band_rows = m2;
      head.band = {band.cfg, band.n_rem, band.nseg, band.ws_bytes};
      consider(head);
    }
  }
  // nothing accepted (every candidate wanted more scratch than the cap allows): whole, unsplit 512-row tiles need none, so the
  // plan always carries a real estimate (a default-constructed plan would price the launch as free for pick_levels / plan_shape)
  if (!have && v8_model(m, l, n, batch, packed, 12, 0, 0, c)) consider(c);
  return best;
}

// fixed cost of the packing pass of a plain product: its launch and the dependent-kernel boundary behind it (4.8 us measured for
// the 2 MiB of a 4096^2 operand, profiles/r03_config2_kernel_stats.csv, of which 0.8 us are the bytes)
static const double kPackLaunch = 5.0e-6;
// the plan of a plain product: A unpacked, or packed by a pass of its own when the model says that pays
PlainPlan plain_plan(int m, int l, int n) {
  static const double bw = (double)dev_env_int("M4RI_HIP_STREAM_GBS", 5000) * 1e9;
  static const int plain_pack = env_int("M4RI_HIP_PLAIN_APACK", 1);
  PlainPlan pp{plan_tiles(m, l, n, 1, false), false, 0.0};
  pp.t = pp.tp.t;
  const long long wp = (words_of(l) + 1) & ~1ll, prow = ((long long)m + 63) & ~63ll;
  if (plain_pack && m >= 512 && prow * wp * 8 < (1ll << 32)) {
    const TilePlan pk = plan_tiles(m, l, n, 1, true);
    const double t = pk.t + 2.0 * (double)prow * (double)wp * 8.0 / bw + kPackLaunch;
    if (cfg_reads_packed(pk.cfg) && t < pp.t) pp = {pk, true, t};
  }
  return pp;
}
static double plain_time_model(int m, int l, int n) { return plain_plan(m, l, n).t; }

// The level plan: a product with L Strassen levels runs L levels of operand splits, ONE batched leaf launch and L levels of
// product merges.  The passes fuse levels so that intermediate operands are never written:
//   step {k, virt}: k (1..3) levels fused in one kernel, operands materialised at the step's end; virt: one more level on
//   top that is never materialised -- the kernel reads the one or two quadrants of the grandparent whose XOR is its source
//   (on the product side the 7 parents of that level are sums in LDS: gf2_strassen_merge4_kernel folds all four levels into C).
//   L: 1 {1}  2 {2}  3 {3}  4 {3 + virtual}  5 {2, 3}  6 {3, 3}          (M4RI_HIP_STRASSEN_FUSE3=0: pairs only, round 1's plan)
std::vector<PlanStep> strassen_plan(int L) {
  const int fuse3 = env_int("M4RI_HIP_STRASSEN_FUSE3", 1);  // read per call: the tests switch plans
  std::vector<PlanStep> p;
  if (L <= 0) return p;
  if (!fuse3) {
    if (L & 1) p.push_back({1, false});
    for (int lv = L & 1; lv < L; lv += 2) p.push_back({2, false});
    return p;
  }
  switch (L) {
    case 1: p = {{1, false}}; break;
    case 2: p = {{2, false}}; break;
    case 3: p = {{3, false}}; break;
    case 4: p = {{3, true}}; break;
    case 5: p = {{2, false}, {3, false}}; break;
    default: p = {{3, false}, {3, false}}; break;  // 6
  }
  return p;
}

// Does the last split pass of an L-level product write the A leaves row-group packed?  (Every split kernel has a packed form --
// the single-level one since round 4 --; the leaf rows must be a multiple of 64; M4RI_HIP_APACK=0 switches the layout off.)
static bool strassen_packs_a(int m, int L) {
  static const int apack_on = env_int("M4RI_HIP_APACK", 1);
  if (!apack_on || L < 1) return false;
  return ((m >> L) & 63) == 0;
}

size_t pow7(int i) {
  size_t p = 1;
  while (i-- > 0) p *= 7;
  return p;
}

// the batched leaf launch of an L-level product (the last split pass may write the A leaves packed): ONE choice, priced by the level
// and shape models, sized by the workspace query and launched by mul_strassen
TilePlan leaf_plan(int m, int l, int n, int L, bool *a_packed) {
  const int batch = (int)pow7(L);
  TilePlan tp = plan_tiles(m >> L, l >> L, n >> L, batch, false);
  bool packed = false;
  if (strassen_packs_a(m, L)) {
    const TilePlan pk = plan_tiles(m >> L, l >> L, n >> L, batch, true);
    if (cfg_reads_packed(pk.cfg) && pk.t <= tp.t) tp = pk, packed = true;
  }
  if (a_packed) *a_packed = packed;
  return tp;
}
// its modelled time.  (Under a forced variant that cannot read packed leaves the packed estimate of plan_tiles still counts, as ever.)
static double leaf_time_model(int m, int l, int n, int L) {
  const double t = leaf_plan(m, l, n, L).t;
  return strassen_packs_a(m, L) ? std::min(t, plan_tiles(m >> L, l >> L, n >> L, (int)pow7(L), true).t) : t;
}

// bytes the split / merge passes of an L-level product move (every kernel reads its sources once and writes its
// destinations once; a virtual level reads 12 quadrants instead of 4)
static double strassen_pass_bytes(double m, double l, double n, int L) {
  double bytes = 0;
  int prev = 0;
  for (const PlanStep &st : strassen_plan(L)) {
    const int i = prev + st.levels();
    const double p7 = (double)pow7(prev);
    const double a_i = (m * l) / std::pow(4.0, i) / 8.0, b_i = (l * n) / std::pow(4.0, i) / 8.0, c_i = (m * n) / std::pow(4.0, i) / 8.0;
    const double rd = st.virt ? 12.0 * std::pow(4.0, st.k) : std::pow(4.0, st.k), wr = std::pow(7.0, st.levels());
    bytes += p7 * (rd + wr) * (a_i + b_i);  // operand sides
    if (st.virt)  // products: the leaves read once and C written once (gf2_strassen_merge4_kernel keeps the 7 parents in LDS)
      bytes += p7 * c_i * (wr + std::pow(4.0, st.k + 1));
    else
      bytes += p7 * c_i * (wr + std::pow(4.0, st.k));
    prev = i;
  }
  return bytes;
}

// number of Strassen levels: `req` > 0 explicit; 0 automatic = the level count with the smallest modelled time
//   t(L) = modelled time of the batched leaf launch (rounds of 256 workgroups x chunks x measured cycles per
//          chunk, split-K included)  +  bytes moved by the split / merge passes / bw
// `leaf_min` bounds the leaf dimensions from below (mzd_mul's cutoff argument, strassen.rs:8-18).
// modelled seconds of the product with exactly L levels on the shape as given (-1: L levels do not divide it)
// fixed cost of one split / merge pass besides its bytes: the dependent-kernel boundary and the ramp of a launch (three passes
// per plan step).  5 us: with 3 us the model preferred two levels at 8192^3 (133 against 138 us), which measures 0.123 against 0.115 ms
static const double kPassLaunch = 5.0e-6;
static double level_time_model(int m, int l, int n, int L) {
  static const double bw = (double)dev_env_int("M4RI_HIP_STREAM_GBS", 5000) * 1e9;        // streaming B/s
  if (L <= 0) return plain_time_model(m, l, n);
  const int d = 1 << L;
  if (L > 6 || m % d || l % (128 * d) || n % (128 * d)) return -1.0;  // leaf rows integral, leaf widths an even word count
  return leaf_time_model(m, l, n, L) + strassen_pass_bytes(m, l, n, L) / bw +
         3 * kPassLaunch * (double)strassen_plan(L).size();
}
extern "C" double gf2_model_time(int m, int l, int n, int levels) { return level_time_model(m, l, n, levels); }

static int pick_levels_uncached(int m, int l, int n, int req, int leaf_min, double *t_out);
int pick_levels(int m, int l, int n, int req, int leaf_min, double *t_out) {
  struct Res {
    int L;
    double t;
  };
  thread_local std::unordered_map<PlanKey, Res, PlanKeyHash> memo;
  const PlanKey key{m, l, n, req, leaf_min * 2 + (env_int("M4RI_HIP_STRASSEN_FUSE3", 1) ? 1 : 0)};  // (the tests switch level plans)
  const Res res = memoised(memo, key, [&] {
    Res r{0, 0.0};
    r.L = pick_levels_uncached(m, l, n, req, leaf_min, &r.t);
    return r;
  });
  if (t_out) *t_out = res.t;
  return res.L;
}
static int pick_levels_uncached(int m, int l, int n, int req, int leaf_min, double *t_out) {
  static const int max_auto = std::min(env_int("M4RI_HIP_STRASSEN_MAX_LEVELS", 5), 6);  // (the level plans end at 6)
  const int cap = req > 0 ? (req > 6 ? 6 : req) : max_auto;
  int best = 0;
  double best_t = 0;
  for (int L = 0; L <= cap; ++L) {
    if (L > 0) {
      const int d = 1 << L;
      if (m % d || l % (128 * d) || n % (128 * d)) break;  // leaf rows integral, leaf widths an even word count
      if (req <= 0 && ((m >> L) < (leaf_min < 1024 ? leaf_min : 1024) || (l >> L) < leaf_min || (n >> L) < leaf_min)) break;
    }
    if (req > 0) {
      best = L;
      continue;
    }
    double t = level_time_model(m, l, n, L);
    // tools/levels_sweep.py (profiles/r03_levels_sweep.txt): the model is 3-10 % pessimistic for 0 and 2 levels and within 3 % for
    // 3 and more, so a further level must promise 1.5 % (up to two levels) / 3 % (beyond) over the best count below it
    if (L == 0 || t < best_t * (L >= 3 ? 0.97 : 0.985)) {
      best = L;
      best_t = t;
    }
  }
  if (t_out) *t_out = best_t;
  return best;
}

// the operand arena, in 64-bit words: operands and products at the end of every step, plus the parents of a virtual level
StrassenArena strassen_arena(int m, int l, int n, int L) {
  StrassenArena ar;
  std::fill_n(ar.a, 7, ar.none), std::fill_n(ar.b, 7, ar.none), std::fill_n(ar.p, 7, ar.none);
  if (L > 6) L = 6;
  int prev = 0;
  for (const PlanStep &st : strassen_plan(L)) {
    const int i = prev + st.levels();
    const size_t mi = (size_t)m >> i, li = (size_t)l >> i, ni = (size_t)n >> i, p7 = pow7(i);
    ar.a[i] = ar.words;
    ar.words += p7 * mi * (li / 64);
    ar.b[i] = ar.words;
    ar.words += p7 * li * (ni / 64);
    ar.p[i] = ar.words;
    ar.words += p7 * mi * (ni / 64);
    if (st.virt) {  // the parents of the virtual level: unused since the four-level merge keeps them in LDS (see mul_plan.h)
      ar.p[prev + 1] = ar.words;
      ar.words += pow7(prev + 1) * ((size_t)m >> (prev + 1)) * (((size_t)n >> (prev + 1)) / 64);
    }
    prev = i;
  }
  return ar;
}

// Few columns against a long inner dimension (`&A * &v` with a large square A; a block of up to 64 vectors): B is transposed
// (n rows of l bits, a few KiB) and a wave per row streams A once (gf2_widevec_kernel), 32 vectors per pass.  The tile kernel
// would compute 512 columns to deliver n (65536^2 times 64 vectors: 1.18 ms against 0.3), the lane-per-row kernels read an
// 8-KiB row 8 bytes at a time per lane (65536^2 times one vector: 0.30 ms against 0.1).
bool widevec_shape(int m, int l, int n) {
  static const int on = dev_env_int("M4RI_HIP_WIDEVEC", 1);
  if (!on || n > 64 || m < 1) return false;
  // Where it wins, from an A/B grid against the older paths on one box (tools/ab_widevec.sh, profiles/r03_widevec_ab.txt;
  // time of the wave-per-row kernel / time of what ran before, at m = 65536 and m = 1000):
  //   n <= 16: l = 2048 0.28-0.48 / 0.8-1.1, 4096 0.37-0.63 / 0.6-0.9, 20000 0.08-0.16 / 0.4-0.6, 65536 0.08-0.16 / 0.4-0.55
  //   n  = 32: l = 4096 1.27 / 0.74, 20000 0.31 / 0.59, 65536 0.30 / 0.97        n = 64: l = 20000 0.63 / 1.04, 65536 0.61 / 1.84
  // (three instructions per vector and word bound it from 9 vectors on; a row per wave needs rows to fill the chip)
  if (m <= 8) return l >= 8192 && (n <= 32 || m >= 4);  // against the v*A kernel: 8 x 65536 x 1 74 -> 9 us, x 64 120 -> 62 us
  static const int minl16 = dev_env_int("M4RI_HIP_WIDEVEC_MINL16", 2048), minl32 = dev_env_int("M4RI_HIP_WIDEVEC_MINL32", 8192);
  // rows of 768 ... 2047 bits: up to 8 vectors and not too many rows (20000 x 1000 x 8: 19 us against 30 for the tile kernel and 44
  // for the generation table kernel; at 2^20 rows the table kernel wins: 86 us against 220)
  if (n <= 8 && l >= 768 && m <= 131072) return true;
  if (n <= 16) return l >= minl16;
  if (n <= 32) return l >= minl32;
  return l >= 16384 && m >= 8192;
}
// up to 64 vectors against a long inner dimension through 4-bit tables rebuilt per 512-bit slab (gf2_tallskinny7_kernel)
bool ts_long_shape(int m, int l, int n) {
  static const int mode = dev_env_int("M4RI_HIP_TS7", 1);  // 0 off, 1 by rule, 2 whenever it can (A/B)
  if (!mode || n > 64 || l <= 256 || m < 1) return false;
  if (mode == 2) return true;
  // Where it wins (tools/ab_ts7.sh, profiles/r03_ts7_ab.txt: its time does not depend on n -- 65536^2: 0.21 ms, 2^20 x 4096: 0.18 ms --
  // while the wave-per-row kernel costs three instructions per vector and word and the tile kernel computes 512 columns):
  //   17-64 vectors: from 2048-bit rows on, or from 16384 rows on (65536^2 x 64: 0.72 -> 0.21 ms; 4096 x 65536 x 64: 92 -> 27 us)
  //    9-16 vectors: many rows and rows of at most 8192 bits (65536 x 4096 x 16: 32 -> 19 us); longer rows stream faster per wave
  //    1-8  vectors: many short rows (2^20 x 1000 x 8: 88 -> 49 us, where the generation table kernel used to run)
  if (n > 16) return l >= 2048 || m >= 16384;
  if (n > 8) return m >= 65536 && l <= 8192;
  return m >= 65536 && l <= 2048;
}
// 9-128 rows against a B much taller than wide: computed transposed (see mul_m4rm_plain)
static bool few_rows_t_shape(int m, int l, int n) {
  static const int few = dev_env_int("M4RI_HIP_FEW_ROWS_T", 1);
  const bool tall = (n >= 1024 && l >= 8 * (long long)n && (long long)l * n >= (1ll << 26) && m <= 64) ||
                    (n > 64 && n <= 1024 && l >= 16384 && l >= 8 * (long long)n && (long long)l * n >= (1ll << 21));
  return few && m > 8 && m <= 128 && tall;
}
static size_t few_rows_t_bytes(int m, int l, int n, int accumulate) {
  const long long ldl = (words_of(l) + 1) & ~1ll, ldn = (words_of(n) + 1) & ~1ll, ldct = ((m + 63) / 64 + 1) & ~1ll;
  return ((size_t)n * ldl + (size_t)l * 2 + (size_t)n * ldct + (accumulate ? (size_t)m * ldn : 0)) * sizeof(u64);
}

PlainPath plain_path(int m, int l, int n) {
  if (m == 0 || n == 0) return kPathNothing;
  if (l == 0) return kPathZeroInner;
  if (ts_long_shape(m, l, n)) return kPathSlabTables;
  {
    static const int mp = dev_env_int("M4RI_HIP_TS7_MULTIPASS", 1);
    static const int maxn = dev_env_int("M4RI_HIP_TS7_MAXN", 256);
    // (129-192 columns would pay a whole second pass for at most 64 of them: 20000 x 40000 x 160 148 -> 165 us)
    static const int minl128 = dev_env_int("M4RI_HIP_TS7_MINL128", 1000);  // (65536 x 1000 x 128: 45 -> 17 us, 262144 x 4096 x 128: 327 -> 82 us)
    if (mp && n > 64 && n <= maxn && (n <= 128 ? m >= 256 && l >= minl128 : n > 192 && m >= 4096 && l >= 32768) && ts_long_shape(m, l, 64))
      return kPathSlabPasses;
  }
  if (widevec_shape(m, l, n)) return kPathWideVec;
  // the table kernels for 256 < l <= 1024 give a workgroup 4096 rows: below 2^19 rows they leave most of the chip idle
  // (65536 x 1000 x 64: 44 us whatever the row count, against 15-45 us through the tile kernel; tools/ab_ts_long.sh)
  static const int ts_long_min_rows = dev_env_int("M4RI_HIP_TS_LONG_MIN_ROWS", 524288);
#ifdef GF2K_DEV_VARIANTS
  constexpr bool has_generation_kernel = true;
#else
  // the shipped gf2k_tallskinny has no kernel for n <= 64 with 256 < l <= 1024 (the slab kernel above takes those shapes under its
  // present thresholds; gf2_tallskinny4_kernel lives in development builds only): should a retuned threshold ever let one through,
  // it goes to the tile kernel instead of failing
  constexpr bool has_generation_kernel = false;
#endif
  if (n <= 256 && m >= (l > 256 ? ts_long_min_rows : 2048) && (n > 64 || l > 64) && l <= 1024 && (has_generation_kernel || n > 64 || l <= 256))
    return kPathTallSkinny;
  if (m <= 8) return kPathFewRows;
  if (few_rows_t_shape(m, l, n)) return kPathFewRowsT;
  return kPathTiles;
}

// Dimensions that do not divide by the level plan (leaf rows integral and a multiple of 64 for the packed layout, leaf widths
// an even word count) keep their Strassen levels in one of two ways (the cliff VERDICT r1 item 4 names: 60000^3 or 65600^3
// would otherwise run as plain M4RM):
//   pad   A and B are copied into zero-padded buffers whose dimensions are rounded UP (one extra pass over each), the product
//         runs on the padded shape and its top left m x n corner is copied / added into C -- right when the dimensions fall
//         a little short of a multiple (60000 -> 61440);
//   peel  the largest dividing core (dimensions rounded DOWN) goes through Strassen in place, the three border strips
//         (bottom rows, right columns, the tail of the inner dimension) through the plain kernels -- right when the dimensions
//         are a little above a multiple (65600 = 65536 + 64: padding would push the 4096-row leaves to two row tiles each).
// The choice is by modelled time against plain M4RM on the given shape.
struct ShapePlan {
  int kind = 0;  // 0 plain, 1 pad, 2 peel
  int L = 0, mp = 0, lp = 0, np = 0;  // padded or core dimensions
  double t = 0;
};
// a border strip runs through the automatic choice among the level counts that divide it (no further padding / peeling)
static double strip_model(int m, int l, int n, int leaf_min) {
  if (m <= 0 || l <= 0 || n <= 0) return 0.0;
  double t = 0;
  (void)pick_levels(m, l, n, 0, leaf_min, &t);
  return t + 3e-6;
}

static ShapePlan plan_shape_uncached(int m, int l, int n, int req, int leaf_min);
static ShapePlan plan_shape(int m, int l, int n, int req, int leaf_min) {
  thread_local std::unordered_map<PlanKey, ShapePlan, PlanKeyHash> memo;
  const PlanKey key{m, l, n, req, leaf_min * 2 + (env_int("M4RI_HIP_STRASSEN_FUSE3", 1) ? 1 : 0)};
  return memoised(memo, key, [&] { return plan_shape_uncached(m, l, n, req, leaf_min); });
}
static ShapePlan plan_shape_uncached(int m, int l, int n, int req, int leaf_min) {
  static const double bw = (double)dev_env_int("M4RI_HIP_STREAM_GBS", 5000) * 1e9;
  static const int max_auto = std::min(env_int("M4RI_HIP_STRASSEN_MAX_LEVELS", 5), 6);  // (the level plans end at 6)
  static const int debug = dev_env_int("M4RI_HIP_DEBUG_PLAN", 0);
  ShapePlan best;
  const double plain = plain_time_model(m, l, n);  // (plan_product asks for m >= 1024, l n >= 2^22)
  best.t = plain;
  if (debug) std::fprintf(stderr, "m4ri_hip plan %d x %d x %d: plain %.3f ms\n", m, l, n, best.t * 1e3);
  const int lo = req > 0 ? (req > 6 ? 6 : req) : 1, hi = req > 0 ? lo : max_auto;
  bool forced_done = false;
  static const int only_kind = dev_env_int("M4RI_HIP_SHAPE_KIND", 0);  // A/B measurements: 1 = padded plans only, 2 = peeled plans only
  auto consider = [&](int kind, int L, long long mm, long long ll, long long nn, double t) {
    if (only_kind && kind != only_kind) return;
    if (debug) std::fprintf(stderr, "  L=%d %s %lld x %lld x %lld: %.3f ms\n", L, kind == 1 ? "pad " : "peel", mm, ll, nn, t * 1e3);
    // (not forced:) the model is coarse: a plan must promise 5 % over plain M4RM to be taken (8 % until the tile model stopped counting
    // the per-tile overhead twice; 30000^3 then sat exactly on the threshold: padded 3.71 ms, plain 4.06 ms measured)
    static const double min_gain = dev_env_int("M4RI_HIP_SHAPE_MIN_GAIN_PCT", 5) * 1e-2;
    if ((req > 0 && !forced_done) || (t < best.t && (req > 0 || t < (1.0 - min_gain) * plain))) best = {kind, L, (int)mm, (int)ll, (int)nn, t}, forced_done = true;
  };
  for (int L = lo; L <= hi; ++L) {
    const long long um = 64ll << L, uw = 128ll << L;
    auto core_time = [&](long long mm, long long ll, long long nn) {
      return leaf_time_model((int)mm, (int)ll, (int)nn, L) +
             strassen_pass_bytes((double)mm, (double)ll, (double)nn, L) / bw + 3 * kPassLaunch * (double)strassen_plan(L).size();
    };
    auto leaves_ok = [&](long long mm, long long ll, long long nn) {
      return req > 0 || ((mm >> L) >= 1024 && (ll >> L) >= leaf_min && (nn >> L) >= leaf_min);
    };
    // pad: round up
    const long long mu = ((long long)m + um - 1) / um * um, lu = ((long long)l + uw - 1) / uw * uw, nu = ((long long)n + uw - 1) / uw * uw;
    if (mu <= 0x7fffffff && lu <= 0x7fffffff && nu <= 0x7fffffff && leaves_ok(mu, lu, nu))
      consider(1, L, mu, lu, nu, core_time(mu, lu, nu) + 2.0 * ((double)mu * lu + (double)lu * nu + (double)mu * nu) / 8.0 / bw + 3 * 3e-6);
    // peel: round down -- to the plan's unit, and to whole tiles of the leaf kernel (4096 rows, 512 columns per leaf: a 4352-row
    // leaf occupies two row tiles, so 70000 is better served by a 65536-row core than by a 69632-row one)
    auto peel = [&](long long md, long long ld, long long nd) {
      if (md <= 0 || ld <= 0 || nd <= 0 || !leaves_ok(md, ld, nd)) return;
      if (md == m && ld == l && nd == n) return;  // the shape as given: pick_levels' business
      // x 1.05: measured against padded plans of the same shapes (60000^3: peeled 26.6 ms at a model of 26.6, padded 25.2 at a model
      // of 26.9; 70000^3: 40.5 / 39.8 and 47.0 / 48.7), the peeled plans run 5-6 % above their model relative to the padded ones
      consider(2, L, md, ld, nd,
               1.05 * (core_time(md, ld, nd) + strip_model((int)md, l - (int)ld, (int)nd, leaf_min) + strip_model((int)md, l, n - (int)nd, leaf_min) +
                       strip_model(m - (int)md, l, n, leaf_min)));
    };
    const long long md = (long long)m / um * um, ld = (long long)l / uw * uw, nd = (long long)n / uw * uw;
    peel(md, ld, nd);
    const long long tm = 4096ll << L, tn = 512ll << L;
    const long long md2 = (long long)m / tm * tm, nd2 = (long long)n / tn * tn;
    if (md2 != md || nd2 != nd) {
      peel(md2 ? md2 : md, ld, nd2 ? nd2 : nd);
      if (md2 && md2 != md && nd2 != nd) peel(md2, ld, nd);
    }
  }
  if (debug) std::fprintf(stderr, "  -> kind %d L=%d (%d x %d x %d) %.3f ms\n", best.kind, best.L, best.mp, best.lp, best.np, best.t * 1e3);
  return best;
}

extern "C" size_t gf2_mul_workspace_bytes(int m, int l, int n, int algo, int param) {
  // the scratch of a plain product follows the path mul_m4rm_plain takes (plain_path): a packed copy of A and partial tiles for
  // the planned tile kernels, the transposed vectors for the wave-per-row kernel, nothing for the table kernels
  auto plain_bytes = [&]() -> size_t {
    switch (plain_path(m, l, n)) {
      case kPathWideVec: return (size_t)n * ((words_of(l) + 1) & ~1) * 8;
      case kPathFewRowsT: return few_rows_t_bytes(m, l, n, 1);
      case kPathTiles: {
        const PlainPlan pp = plain_plan(m, l, n);
        return pp.tp.scratch() + (pp.pack ? (size_t)((m + 63) & ~63) * (size_t)((words_of(l) + 1) & ~1) * 8 : 0);
      }
      default: return 0;
    }
  };
  if (algo == GF2_ALGO_NAIVE) {
    // mul_naive_dev: wide products are forwarded to mul_m4rm_plain; up to 64 columns take the table / wave-per-row kernels or the
    // AND / popcount kernels, which need at most the transposed B
    if (n > 64 || l == 0) return plain_bytes();
    if (m > 0 && ts_long_shape(m, l, n)) return 0;
    if (m > 0 && widevec_shape(m, l, n)) return (size_t)n * ((words_of(l) + 1) & ~1) * 8;
    if (n > 8 && m >= 2048) return plain_bytes();
    return (size_t)n * ((words_of(l) + 1) & ~1) * 8;
  }
  const size_t plain_ws = plain_bytes();
  if (algo == GF2_ALGO_M4RM) return plain_ws;
  const int L = pick_levels(m, l, n, param, strassen_leaf_min());
  if (L <= 0) return plain_ws;
  return strassen_arena(m, l, n, L).words * sizeof(u64) + leaf_plan(m, l, n, L).scratch();
}

extern "C" double gf2_strassen_pass_bytes(int m, int l, int n, int levels) {
  return levels > 0 ? strassen_pass_bytes(m, l, n, levels) : 0.0;
}

extern "C" double gf2_tile_plan(int m, int l, int n, int batch, int packed, long long out[9]) {
  const TilePlan tp = plan_tiles(m, l, n, batch < 1 ? 1 : batch, packed != 0);
  const long long v[9] = {tp.cfg, tp.ksplit, tp.n_rem, tp.nseg, (long long)tp.scratch(), tp.tail_batch, tp.tail.cfg, tp.tail.n_rem, tp.tail.nseg};
  if (out) std::copy(v, v + 9, out);
  return tp.t;
}

// the row band of the same plan: out = {rows of the band (0: none), its variant, its stream-K cut (tiles, segments), its scratch}
extern "C" void gf2_tile_plan_band(int m, int l, int n, int batch, int packed, long long out[5]) {
  if (!out) return;
  const TilePlan tp = plan_tiles(m, l, n, batch < 1 ? 1 : batch, packed != 0);
  const long long v[5] = {tp.band_rows, tp.band.cfg, tp.band.n_rem, tp.band.nseg, (long long)tp.band.ws_bytes};
  std::copy(v, v + 5, out);
}

// What a Strassen / automatic product of this shape runs (mul_plan.h): gf2_mul_dispatch executes it, gf2_mul_plan reports it.
MulPlan plan_product(int m, int l, int n, int param, bool even_strides) {
  static const int pad_on = env_int("M4RI_HIP_STRASSEN_PAD", 1);
  MulPlan mp{0, 0, {m, l, n}, 0};
  mp.L = mp.L_given = pick_levels(m, l, n, param, strassen_leaf_min());
  const bool divides = mp.L > 0 && (param <= 0 || mp.L == (param > 6 ? 6 : param)) && even_strides;
  if (pad_on && !divides && m >= 1024 && (long long)l * n >= (1ll << 22)) {  // lost levels to divisibility (or to odd strides)?
    ShapePlan pp = plan_shape(m, l, n, param, strassen_leaf_min());
    if (pp.kind == 2 && !even_strides) pp.kind = 0;  // peeling works on views of the caller's buffers
    if (pp.kind && pp.L > mp.L) mp = {pp.kind, pp.L, {pp.mp, pp.lp, pp.np}, mp.L_given};
  }
  return mp;
}

// How a device product of this shape would run (no device needed: the cost model's answer, before the memory cap):
// *kind = 0 as given (levels Strassen levels, 0 = plain M4RM), 1 zero-padded to dims[0..2], 2 peeled to the core dims[0..2]
// with the border strips through the plain kernels.  Returns the number of Strassen levels.
extern "C" int gf2_mul_plan(int m, int l, int n, int algo, int param, int *kind, int dims[3]) {
  MulPlan mp{0, 0, {m, l, n}, 0};
  if (algo == GF2_ALGO_AUTO || algo == GF2_ALGO_STRASSEN) mp = plan_product(m, l, n, param);
  if (kind) *kind = mp.kind;
  if (dims) dims[0] = mp.d[0], dims[1] = mp.d[1], dims[2] = mp.d[2];
  return mp.L;
}

// ---- schedules of a large host product (round 5) ----
// Modelled device time of one (sub-)product as the host path would run it.
static double host_product_model(int m, int l, int n, int algo, int param) {
  if (algo == GF2_ALGO_M4RM || algo == GF2_ALGO_NAIVE) return plain_time_model(m, l, n);
  double t = 0;
  (void)pick_levels(m, l, n, param, strassen_leaf_min(), &t);
  return t > 0 ? t : plain_time_model(m, l, n);
}
// A host product is three queues -- uploads, products, downloads -- and a plan is the order and size of their pieces.  Two families:
//   row blocks   C_i = A_i B: blocks of A and C (the first one against the two halves of B, so that it can start early); every
//                block's rows of C leave as soon as they exist, but a block product runs below the whole product's efficiency
//                (8192-row blocks of 32768^3: 1.45 ms against 1.0 for a quarter of the whole);
//   slabs        C ^= A[:, K] B[K, :] over slabs K of the INNER dimension: every product keeps all rows (65536 x 16384 x 65536
//                accumulate: 8.4 ms, a quarter of the whole product is 7.2), only the first slab's upload is exposed -- A's
//                slab is a 2-D copy of 1-2 KiB pieces, which runs at the linear rate --; the last slab is multiplied in row
//                blocks so that C does not leave all at once behind it.
// Which one ends first depends on how compute and PCIe compare, so each candidate is played through with the planner's own time
// model and the copy rate of the link (profiles/r05_slab_prices.txt has the measured sub-products).
constexpr int kHostPlanCandidates = 12;
HostPlan plan_host_product(int rows, int l, int n, int algo, int param, bool b_resident, size_t a_row_bytes, size_t b_row_bytes, size_t c_row_bytes,
                           double *all_t_end, int *chosen) {
  static const double rate = (double)dev_env_int("M4RI_HIP_PCIE_GBS", 55) * 1e9;
  // read per call (tests and A/B runs): the number of a candidate below (1 row blocks ... 12); 0 = by the model
  const int forced = env_int("M4RI_HIP_HOST_PLAN", 0);
  auto T = [&](int m_, int l_) { return host_product_model(m_, l_, n, algo, param); };
  const int NB = 4;
  // row blocks: quarter, half, quarter when a quarter keeps 16384 rows (see host_mul_range), B in two halves for the first block
  HostPlan rb;
  {
    const int q = rows / 4;
    std::vector<int> bnd = q >= 16384 ? std::vector<int>{0, q, 3 * q, rows} : std::vector<int>{0, q, 2 * q, 3 * q, rows};
    const bool halves = !b_resident && l >= 8192 && l % 256 == 0;
    double up = 0, tc = 0, td = 0;
    std::vector<double> arrA;
    up += (double)bnd[1] * a_row_bytes / rate;
    arrA.push_back(up);
    double bt = up, bb = up;
    if (!b_resident) {
      up += (double)l / 2 * b_row_bytes / rate;
      bt = up;
      up += (double)l / 2 * b_row_bytes / rate;
      bb = up;
    }
    for (size_t i = 1; i + 1 < bnd.size(); ++i) {
      up += (double)(bnd[i + 1] - bnd[i]) * a_row_bytes / rate;
      arrA.push_back(up);
    }
    for (size_t i = 0; i + 1 < bnd.size(); ++i) {
      const int R = bnd[i + 1] - bnd[i];
      if (i == 0 && halves) {
        tc = std::max(tc, std::max(arrA[0], bt)) + T(R, l / 2);
        tc = std::max(tc, bb) + T(R, l / 2);
      } else {
        tc = std::max(tc, std::max(arrA[i], bb)) + T(R, l);
      }
      td = std::max(td, tc) + (double)R * c_row_bytes / rate;
    }
    rb.t_end = td;
  }
  auto slab_plan = [&](const std::vector<std::vector<int>> &gs) {
    HostPlan hp;
    hp.gslabs = gs;
    const int NR = (int)gs.size(), rg = rows / NR;
    double up = 0, tc = 0, td = 0;
    for (int g = 0; g < NR; ++g) {
      const std::vector<int> &ks = gs[g];
      for (size_t si = 0; si < ks.size(); ++si) {
        up += ((double)rg * ks[si] / 8.0 + ((b_resident || g > 0) ? 0.0 : (double)ks[si] * b_row_bytes)) / rate;
        if (si + 1 < ks.size() || g + 1 < NR) {
          tc = std::max(tc, up) + T(rg, ks[si]);
          if (si + 1 == ks.size()) td = std::max(td, tc) + (double)rg * c_row_bytes / rate;
        } else {
          for (int b = 0; b < NB; ++b) {
            tc = std::max(tc, up) + T(rg / NB, ks[si]);
            td = std::max(td, tc) + (double)(rg / NB) * c_row_bytes / rate;
          }
        }
      }
    }
    hp.t_end = td;
    return hp;
  };
  // the candidates, in the numbering of M4RI_HIP_HOST_PLAN (a candidate that does not apply to the shape keeps its number, t_end < 0)
  const bool slabs_ok = l % (8 * 1024) == 0 && l >= 16384 && rows % (NB * 64) == 0;
  const bool two_ok = slabs_ok && rows % (2 * NB * 64) == 0 && rows / 2 >= 8192;
  const bool fine_ok = l % (16 * 1024) == 0;  // sixteenths of the inner dimension stay multiples of 1024 bits
  const std::vector<int> E4{l / 4, l / 4, l / 4, l / 4}, H2{l / 2, l / 2}, W1{l}, G8{l / 8, l / 8, l / 4, l / 2},
      G16{l / 16, l / 16, l / 8, l / 4, l / 4, l / 4};
  HostPlan none;
  none.t_end = -1.0;
  std::vector<HostPlan> cands{rb};
  cands.push_back(slabs_ok ? slab_plan({E4}) : none);                       // 2
  cands.push_back(slabs_ok ? slab_plan({G8}) : none);                       // 3
  cands.push_back(slabs_ok ? slab_plan({H2}) : none);                       // 4
  cands.push_back(two_ok ? slab_plan({E4, E4}) : none);                     // 5
  cands.push_back(two_ok ? slab_plan({H2, H2}) : none);                     // 6
  cands.push_back(two_ok && fine_ok ? slab_plan({G16, H2}) : none);         // 7
  cands.push_back(two_ok && fine_ok ? slab_plan({G16, E4}) : none);         // 8
  cands.push_back(two_ok ? slab_plan({G8, H2}) : none);                     // 9
  cands.push_back(two_ok ? slab_plan({E4, H2}) : none);                     // 10
  cands.push_back(slabs_ok && fine_ok ? slab_plan({G16}) : none);           // 11
  cands.push_back(two_ok && fine_ok ? slab_plan({G16, W1}) : none);         // 12
  static_assert(kHostPlanCandidates == 12, "candidate list");
  if (all_t_end)
    for (size_t i = 0; i < (size_t)kHostPlanCandidates; ++i) all_t_end[i] = i < cands.size() ? cands[i].t_end : -1.0;
  // the fastest slab plan by the model -- within half a percent the LATER candidate wins: two row groups measured 0.2-0.3 ms ahead
  // of their one-group twins where the model has them level (32768^3 7.9 against 8.2 ms, 65536^3 41.0 against 41.4; profiles/
  // r05_host_plan_ab.txt) --, taken if it promises 3 % over the row blocks
  size_t best = 0, bs = 0;
  for (size_t i = 1; i < cands.size(); ++i)
    if (cands[i].t_end > 0 && (!bs || cands[i].t_end <= 1.005 * cands[bs].t_end)) bs = i;
  if (bs && cands[bs].t_end < 0.97 * cands[0].t_end) best = bs;
  if (forced >= 1 && forced <= (int)cands.size() && cands[(size_t)forced - 1].t_end > 0) best = (size_t)forced - 1;
  if (chosen) *chosen = (int)best + 1;
  return cands[best];
}

// The schedules a large product on HOST matrices can take, as the library's time model plays them through (plan_host_product):
// t_end[i] = modelled seconds of schedule i + 1 in M4RI_HIP_HOST_PLAN's numbering (-1: not applicable to this shape); returns the
// number of the schedule the host path takes (0: the product is not pipelined at all).  Plain row-major operands of the natural strides.
extern "C" int gf2_host_plan_model(int m, int l, int n, int algo, int param, double t_end[12]) {
  for (int i = 0; i < kHostPlanCandidates; ++i) t_end[i] = -1.0;
  if (m < 16384 || m % 256 || (long long)l * n < (1ll << 28)) return 0;
  auto stride = [](int c) { const size_t w = (size_t)(c + 63) / 64; return (w < 3 || (w & 1) == 0 ? w : w + 1) * sizeof(word); };
  int chosen = 0;
  (void)plan_host_product(m, l, n, algo, param, false, stride(l), stride(n), stride(n), t_end, &chosen);
  return chosen;
}

