// api_internal.h -- the runtime every translation unit of the library shares (runtime_host.cpp unless noted): error state, pooled
// device memory, per-stream scratch, streams, and the host <-> device copies, and nothing else: the launch planner has its own header
// (mul_plan.h), the argument and aliasing rules of the device-resident entries theirs (dev_args.h).
#pragma once
[[noreturn]] void gf2_die(const char *msg);
#include "../../include/m4ri_hip.h"
#include <hip/hip_runtime.h>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
mzd_t *gf2_mzd_init_uncleared(rci_t r, rci_t c);  // mzd_init without the memset (callers overwrite every word)
// GPU-backed transpose of a host matrix (upload, 64x64-block kernel, download); 0 on success.  Used by mzd_transpose
// for large matrices; the caller falls back to the host routine if it fails (this is not the multiply path).
int gf2_host_transpose_gpu(mzd_t *dst, mzd_t const *src);
extern "C" int gf2_device_count(void);
// drop the device copy kept for M by gf2_mzd_cache_on_device, if any (mzd_free and every in-place writer call this)
void gf2_cache_forget(mzd_t const *M);
// size dispatch of the drop-in entry points (gf2_small_host.cpp): M4RI_HIP_HOST_SMALL_WORK word operations, 0 = never
long long gf2_small_work_limit();
bool gf2_small_product(long long m, long long l, long long n);
// pinned scratch blocks from the pool of mzd_host.cpp (null without a device)
void *gf2_pinned_alloc(size_t bytes);
void gf2_pinned_free(void *p, size_t bytes);
// mzd_transpose(DST, A) served from the packed side copy a fresh thin product carries (m4ri_hip_api.cpp, ResultSide): the
// destination (allocated when DST is NULL), or nullptr when A has no side copy
mzd_t *gf2_transpose_from_side_copy(mzd_t *DST, mzd_t const *A);
bool gf2_mzd_block_is_pinned(mzd_t const *M);
// error reporting: set gf2_last_error and return the error code
int gf2_fail_msg(const char *what);
int gf2_fail_hip(hipError_t e, const char *what);
#define HIP_TRY(expr)                                       \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return gf2_fail_hip(_e, #expr);   \
  } while (0)
#define GF2_RC(expr)     \
  do {                   \
    int _rc = (expr);    \
    if (_rc) return _rc; \
  } while (0)
int gf2_require_device();  // 0, or the "no usable HIP device" error
// scratch from the per-stream arena (grown on demand, reused by later calls on the stream, released by gf2_trim).  A slot belongs to one
// user: two that named the same one would share an arena on a stream.
enum Gf2ScratchSlot {
  GF2_SLOT_OPERANDS = 0,               // Strassen operand arena / transposed operand of the naive entry
  GF2_SLOT_PARTIAL_TILES = 1,          // split-K and stream-K partial tiles
  GF2_SLOT_PACKED_A = 2,               // packed A
  GF2_SLOT_PADDED = 3,                 // the copies of a padded product
  GF2_SLOT_TRSM_INVERSES = 4,          // gf2_trsm.hip: block inverses
  GF2_SLOT_TRSM_LEAF = 5,              // gf2_trsm.hip: a leaf's result
  GF2_SLOT_GATHER_TRANSPOSED = 6,      // gather/gather_host.cpp: S^T
  GF2_SLOT_GATHER_ROWS = 7,            // gather/gather_host.cpp: the gathered rows of the composed column gather
  GF2_SLOT_WEIGHT_COL_PARTIALS = 8,    // weight/weight_host.cpp: per-band column sums
  GF2_SLOT_WEIGHT_SELECT_COUNTS = 9,   // weight/weight_host.cpp: block counts of the selection
  GF2_SLOT_WHT_MIN_PARTIALS = 10,      // wht/wht_host.cpp: the per-workgroup minima of gf2_min_weight_dev
  GF2_SLOT_BKW_BLOCK_COUNTS = 11,      // bkw/bkw_host.cpp: block counts of the compaction of gf2_lf1_reduce_dev
  GF2_SLOT_LF2_SORT = 12,              // lf2/lf2_host.cpp: pair buffers and digit counts of the class sort
  GF2_SLOT_LF2_PAIRS = 13,             // lf2/lf2_host.cpp: sorted order, sorted keys and run sums of gf2_lf2_reduce_dev
  GF2_SLOT_DRAW_PERM = 14,             // draw/draw_host.cpp: pair buffers and digit counts of the sort of gf2_draw_permutation_dev
  GF2_SLOT_JOIN = 15,                  // join/join_host.cpp: the sorts' work space, sorted orders and keys of A and B, run sums of gf2_join_dev
  GF2_SLOT_NEAR = 16,                  // near/near_host.cpp: the cells (row of A, chunk of B) of gf2_near_pairs_dev and gf2_nearest_dev
  GF2_SLOT_UNIQUE = 17,                // unique/unique_host.cpp: the sort's work space, run carries, sorted order and block counts of gf2_sort_rows_dev / gf2_unique_rows_dev
  GF2_SLOT_FIND = 18,                  // find/find_host.cpp: the hash table (entries, member counts) of gf2_find_rows_dev
  GF2_SLOT_JOIN_ROWS = 19,             // join_rows/join_rows_host.cpp: the table over B, rep, class starts, the sort's work space, sorted order, idx, mult, offsets and run sums of gf2_group_rows_dev / gf2_join_rows_dev
};
int gf2_stream_scratch(hipStream_t s, size_t bytes, void **out, int slot);  // slot: a Gf2ScratchSlot
// counts a run of a host routine of the size dispatch (gf2_host_small_calls)
void gf2_note_host_small_call();
// pooled device memory.  gf2_dev_free is NOT stream-ordered: the caller guarantees that no queued work still touches the block (it
// synchronised its stream, or it goes through gf2_dmat_free / gf2_dmat_free_async)
int gf2_dev_alloc(void **p, size_t bytes);
void gf2_dev_free(void *p, size_t bytes);
// what an arena on stream s may grow to: 95 % of what the driver reports free plus what the library holds for it already (the block
// cache and the stream's slot 0 are handed back before a larger arena is allocated); SIZE_MAX when the driver does not say
size_t gf2_dev_arena_limit(hipStream_t s);
struct DevBuf {  // a pooled block for the length of a scope
  void *p = nullptr;
  size_t bytes = 0;
  int alloc(size_t b) {
    bytes = b ? b : 8;
    return gf2_dev_alloc(&p, bytes);
  }
  ~DevBuf() { gf2_dev_free(p, bytes); }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
};
int gf2_private_stream(hipStream_t *out);  // the calling thread's own stream on the current device (host entry points)
// Side streams + events for one main stream (copy streams of the host pipelines); cached per (device, stream), never destroyed
struct SideStream {
  hipStream_t s2 = nullptr;
  hipStream_t s3 = nullptr;  // second copy stream of the host pipeline (downloads; s2 carries the uploads)
  std::vector<hipEvent_t> ev;
};
int gf2_side_stream(hipStream_t s, int nevents, SideStream **out, bool want_s3 = false);
// Products that use the per-stream workspace enqueue several kernels that must stay contiguous on the stream
// (another host thread enqueueing on the SAME stream in between would reuse the arena under them).
extern std::mutex gf2_enqueue_mu;
// bench.py's roofline: HIP events on the launch stream around the tile-kernel launches of one (batched) product
struct ProfScope {
  hipEvent_t a{}, b{};
  bool on = false;
  hipStream_t s;
  explicit ProfScope(hipStream_t s_);
  ~ProfScope();
};
bool gf2_prof_is_on();  // gf2_prof_enable's switch (gf2_nullspace.hip times its assembly launch while it is on)

// device matrices <-> host mzd_t
static inline long long dev_ld_for(int ncols) {
  const long long w = ((long long)ncols + 63) >> 6;
  return w <= 1 ? (w ? w : 1) : ((w + 1) & ~1ll);
}
void gf2_dmat_release(gf2_dmat *M);  // gf2_dmat_free without the wait: the caller has waited for every stream that touched M
// rows [r0, r0 + dst->nrows) of src -> dst; asynchronous: `src` must stay untouched until the stream has passed the copy
int gf2_upload_rows_async(gf2_dmat *dst, mzd_t const *src, int r0, hipStream_t s);
// src -> rows [r0, r0 + src->nrows) of a host matrix; returns when they are complete in host memory
int gf2_download_rows(mzd_t *dst, int r0, gf2_dmat const *src, hipStream_t s);

// the products on device matrices (mul_dev_host.cpp); gf2_mul_dispatch takes gf2_enqueue_mu unless sync_free (a private stream)
int gf2_mul_m4rm_plain(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, hipStream_t s);
int gf2_mul_dispatch(gf2_dmat *C, const gf2_dmat *A, const gf2_dmat *B, int accumulate, int algo, int param, hipStream_t s, bool sync_free);

// host operands on the device (m4ri_hip_api.cpp)
struct CachedOperand;
struct DMatOwner {
  gf2_dmat d{};
  std::shared_ptr<CachedOperand> borrowed;  // d belongs to the operand cache, kept alive by this reference
  bool released = false;                    // ownership moved elsewhere
  ~DMatOwner() {
    if (!borrowed && !released) gf2_dmat_release(&d);  // every user synchronises its stream before the owner goes out of scope
  }
};
std::shared_ptr<CachedOperand> gf2_cache_lookup(const mzd_t *M);
// device copy of rows [r0, r1) of M (of all of M) whose row stride equals the host row stride when the host block is contiguous
int gf2_to_device_rows(DMatOwner &o, const mzd_t *M, int r0, int r1, hipStream_t s, bool copy);
int gf2_to_device(DMatOwner &o, const mzd_t *M, hipStream_t s, bool copy);
// M4RI_HIP_DEVICES = one ordinal: every host entry point runs on that device.  RAII: sets it, restores the caller's.
struct PinnedDevice {
  int prev = -1;
  bool switched = false;
  PinnedDevice();
  ~PinnedDevice();
  PinnedDevice(const PinnedDevice &) = delete;
  PinnedDevice &operator=(const PinnedDevice &) = delete;
};

// the reduced row echelon form of gf2_echelonize_dev(full = 1, all columns) that also hands over the elimination's device array of pivot
// columns: *pivcols_dev (null when the matrix is empty) is released with gf2_dev_free(*pivcols_dev, *pivcols_bytes); pivcols_host may
// be null.  Synchronous on s.  (elim_host.cpp)
int gf2_rref_keep_pivots_dev(gf2_dmat *A, int *rank, int *pivcols_host, void **pivcols_dev, size_t *pivcols_bytes, hipStream_t s);
