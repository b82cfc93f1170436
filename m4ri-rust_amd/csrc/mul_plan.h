// mul_plan.h -- the launch planner (mul_plan_host.cpp): what a product of a given shape runs, and its modelled time.  Pure host
// arithmetic on the shape and the environment: no HIP header, no device.  The units that launch (mul_dev_host.cpp, m4ri_hip_api.cpp)
// execute these plans; the exported queries (gf2_tile_plan, gf2_mul_plan, gf2_mul_workspace_bytes, ...) report them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "gf2_env.h"
#include "gf2_variants.h"

int strassen_leaf_min();  // M4RI_HIP_STRASSEN_LEAF_MIN, read once

// ---- which tile kernel, and how its launch is cut ----
struct TilePlan {
  int cfg = 7;
  int ksplit = 1;           // v3 / v6: uniform slices of the inner dimension
  int n_rem = 0, nseg = 0;  // v8: tiles cut into stream-K segments, number of segments
  bool packed = false;
  double t = 0;             // modelled seconds of the launch (reduction of partial tiles included)
  size_t ws_bytes = 0;      // scratch for partial tiles
  // a batched launch may be cut in two: the first `batch - tail_batch` products as planned above (whole rounds of 256 tiles), the
  // last tail_batch products in a launch of their own with its own variant and split (a short tile height, every tile cut)
  struct Part { int cfg = 0, n_rem = 0, nseg = 0; size_t ws_bytes = 0; };  // a launch of its own: variant, stream-K cut, scratch
  int tail_batch = 0;
  Part tail;
  // the rows below the last whole tile row of the main launch may run as a launch of their own with a shorter tile (a "row
  // band": 17000 rows = four tile rows of 4096 + 616 rows in 1024-row tiles instead of a fifth tile row that is 15 % full)
  int band_rows = 0;
  Part band;
  size_t scratch() const { return std::max(ws_bytes, std::max(tail.ws_bytes, band.ws_bytes)); }  // the launches run one after the other
};
enum { PLAN_TAIL = 2, PLAN_BAND = 4, PLAN_V8_ONLY = 8 };  // what a plan may contain (PlanKey::flags; bit 0 = packed A)
// `packed`: A is handed over row-group packed (Strassen leaves, or a plain product that packs A itself).  Memoised per thread.
TilePlan plan_tiles(int m, int l, int n, int batch, bool packed, int mode = PLAN_TAIL | PLAN_BAND);
// the plan of a plain product: A unpacked, or packed by a pass of its own (`pack`) when the model says that pays; t: the modelled
// seconds of the product, packing pass included
struct PlainPlan { TilePlan tp; bool pack; double t; };
PlainPlan plain_plan(int m, int l, int n);

// Which kernel family a plain (no Strassen) product takes -- ONE decision, used by gf2_mul_m4rm_plain and by
// gf2_mul_workspace_bytes (the query had drifted from the dispatch order).
enum PlainPath {
  kPathNothing,      // an empty operand
  kPathZeroInner,    // l == 0: C is zero
  kPathSlabTables,   // gf2k_tallskinny_long: up to 128 columns against a long inner dimension, no scratch
  kPathSlabPasses,   // the same in passes of 128 columns
  kPathWideVec,      // a wave per row: scratch = the transposed vectors
  kPathTallSkinny,   // tables over all of B in LDS (l <= 1024): no scratch
  kPathFewRows,      // m <= 8: v*A kernel, no scratch
  kPathFewRowsT,     // 9-128 rows against a tall B, computed transposed: scratch = few_rows_t_bytes
  kPathTiles         // the planned tile kernels (maybe a packed copy of A and stream-K / split-K partial tiles)
};
PlainPath plain_path(int m, int l, int n);
bool widevec_shape(int m, int l, int n);
bool ts_long_shape(int m, int l, int n);

// ---- Strassen levels ----
struct PlanStep {
  int k;
  bool virt;
  int levels() const { return k + (virt ? 1 : 0); }
};
std::vector<PlanStep> strassen_plan(int L);
size_t pow7(int i);
// The operand arena of an L-level product: word offsets of the operands (a, b) and products (p) of every level at which a plan step
// ends -- p also for the parents of a virtual level --, and the total.  The workspace query sizes it, mul_strassen carves it.
// The slots of a virtual level's parents go unused: gf2_strassen_merge4_kernel folds the leaves straight into C and never writes
// them.  They stay in the arena because the workspace a caller was told to provide is part of the interface.
struct StrassenArena {  // (L <= 6: pick_levels and plan_product never give more)
  static constexpr size_t none = ~(size_t)0;  // a level the plan does not materialise
  size_t a[7], b[7], p[7], words = 0;
};
StrassenArena strassen_arena(int m, int l, int n, int L);
// the batched leaf launch of an L-level product of m x l x n: its A leaves packed by the last split pass (*a_packed) if that is faster
TilePlan leaf_plan(int m, int l, int n, int L, bool *a_packed = nullptr);
// number of Strassen levels for the shape as given: `req` > 0 explicit, 0 = the count with the smallest modelled time (*t_out)
int pick_levels(int m, int l, int n, int req, int leaf_min, double *t_out = nullptr);
// What a product of this shape runs, before the memory cap: kind 0 as given (L levels, 0 = plain M4RM), 1 zero-padded to d, 2 peeled to
// the core d with the border strips plain; L_given: the levels of the shape as given (what runs if that arena does not fit).
struct MulPlan { int kind, L, d[3], L_given; };
MulPlan plan_product(int m, int l, int n, int param, bool even_strides = true);

// ---- schedules of a large product on host matrices ----
struct HostPlan {
  // slab plans: gslabs[g] = the sizes (bits) of the slabs of the inner dimension through which row group g of A and C runs, one group
  // after the other (a finished group's rows of C leave while the next group is multiplied; half-height sub-products are no less
  // efficient: 32768^3 16384 x 8192 x 32768 0.64 ms against 1.24 for twice the rows).  The FIRST group's slabs also bring B in, so
  // they start small (a short lead-in) and grow; later groups find B resident and take few, large slabs.  Empty: the row-block plan.
  std::vector<std::vector<int>> gslabs;
  double t_end = 0;
};
HostPlan plan_host_product(int rows, int l, int n, int algo, int param, bool b_resident, size_t a_row_bytes, size_t b_row_bytes, size_t c_row_bytes,
                           double *all_t_end = nullptr, int *chosen = nullptr);
