// gf2_variants.h -- what the launch planner (mul_plan_host.cpp) and the launchers (gf2_kernels.hip) must agree on, kept once: the
// geometry of every tile-kernel variant, the stream-K cut of a v8 launch and the Strassen combination tables.  Plain C++ without a
// HIP header: tests/cpp/test_streamk_cut.cpp compiles it with g++ and checks the cut exhaustively.
#pragma once

// cfg (shipped): 7 = v3 1024 x 2048 tile, 20 = v3 256 x 2048 (4 waves), 8 = v6 2048 x 1024, 81 / 82 = v6 with a deeper / shallower
// read window, 9 / 10 / 11 / 12 = v8 with 4096 / 2048 / 1024 / 512-row tiles of 512 columns.  Development builds (-DGF2K_DEV_VARIANTS)
// add 13-19 = v8 with a read window of three steps / one step, 21 / 22 / 23 = v9 with 4096 / 2048 / 1024-row tiles of 128 columns,
// 90-99 = the legacy v7, 8x = v5 / v6 ablations, 0 / 1 = the first generation.
struct gf2_variant {
  int rows, cols;     // bits of C per tile
  int v8_rg, v9_rg;   // v8 / v9 family: row groups of 512 rows per tile (0: another family)
  bool reads_packed;  // takes A row-group packed (gf2k_mul_args::a_packed)
  bool shipped;       // exists in libm4ri_hip.so and computes the product (M4RI_HIP_M4RM_CFG accepts it)
};
inline gf2_variant gf2_variant_of(int cfg) {
  gf2_variant v{1024, 2048, 0, 0, false, false};
  v.v8_rg = cfg >= 9 && cfg <= 12 ? 8 >> (cfg - 9) : 0;
#ifdef GF2K_DEV_VARIANTS
  if (cfg >= 13 && cfg <= 16) v.v8_rg = 8 >> (cfg - 13);
  if (cfg >= 17 && cfg <= 19) v.v8_rg = 8 >> (cfg - 17);
  v.v9_rg = cfg >= 21 && cfg <= 23 ? 8 >> (cfg - 21) : 0;
#endif
  const bool v7 = v.v8_rg > 0 || (cfg >= 90 && cfg < 100), v56 = cfg == 8 || (cfg >= 80 && cfg < 90);
  v.rows = v.v8_rg ? 512 * v.v8_rg : v.v9_rg ? 512 * v.v9_rg : (cfg == 1 || cfg == 20) ? 256 : v7 ? 4096 : v56 ? 2048 : 1024;
  v.cols = v.v9_rg ? 128 : v7 ? 512 : v56 ? 1024 : 2048;
  v.reads_packed = cfg == 8 || v7 || v.v9_rg > 0;
  v.shipped = cfg == 7 || cfg == 8 || (cfg >= 9 && cfg <= 12) || cfg == 20 || cfg == 81 || cfg == 82;
  return v;
}

// Stream-K cut of a v8 launch of T tiles with Q units of the inner dimension each: the last n_rem tiles (clamped to T) are cut into
// about `want` (< 1: 256) segments of `seg` units, 1 <= seg <= Q, so that a segment spans at most two tiles; nseg = ceil(n_rem Q / seg).
// n_rem == 0 in the result: the cut is void (no tiles asked for, or no tile would be cut: whole tiles only).
struct gf2_streamk_cut {
  long long n_rem, nseg, seg;
};
inline gf2_streamk_cut gf2_streamk_cut_of(long long T, long long Q, long long n_rem, long long want) {
  if (n_rem > T) n_rem = T;
  if (n_rem <= 0 || Q < 1) return {0, 0, 0};
  if (want < 1) want = 256;
  const long long gtot = n_rem * Q;
  long long seg = (gtot + want - 1) / want;
  if (seg > Q) seg = Q;
  if (seg < 1) seg = 1;
  const long long nseg = (gtot + seg - 1) / seg;
  if (nseg <= n_rem && seg == Q) return {0, 0, 0};
  return {n_rem, nseg, seg};
}
// 64-bit words of partial-tile scratch a cut into nseg segments needs: two slots of one tile (rows x 8 words; v9: x 2) per segment
inline long long gf2_streamk_words(const gf2_variant &v, long long nseg) {
  return v.v9_rg ? 2 * nseg * v.rows * 2 : v.v8_rg ? 2 * nseg * v.rows * 8 : 0;
}

// Strassen: quadrants (0 = X11, 1 = X12, 2 = X21, 3 = X22) that combination q of a side adds up; second entry -1: a plain copy.
// One initialiser for the device table of the split kernels and the host table of the virtual level (mul_dev_host.cpp).
//   A side: A11+A22, A21+A22, A11, A22, A11+A12, A21+A11, A12+A22    B side: B11+B22, B11, B12+B22, B21+B11, B22, B11+B12, B21+B22
#define GF2_STRASSEN_SUPP \
  {{{0, 3}, {2, 3}, {0, -1}, {3, -1}, {0, 1}, {2, 0}, {1, 3}}, {{0, 3}, {0, -1}, {1, 3}, {2, 0}, {3, -1}, {0, 1}, {2, 3}}}
