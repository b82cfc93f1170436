// api_internal.h -- shared between mzd_host.cpp and m4ri_hip_api.cpp
#pragma once
[[noreturn]] void gf2_die(const char *msg);
#include "../../include/m4ri_hip.h"
#include <hip/hip_runtime.h>
mzd_t *gf2_mzd_init_uncleared(rci_t r, rci_t c);  // mzd_init without the memset (callers overwrite every word)
// GPU-backed transpose of a host matrix (upload, 64x64-block kernel, download); 0 on success.  Used by mzd_transpose
// for large matrices; the caller falls back to the host routine if it fails (this is not the multiply path).
int gf2_host_transpose_gpu(mzd_t *dst, mzd_t const *src);
int gf2_device_count(void);
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
// error reporting of the other translation units (gf2_ple.hip): set gf2_last_error and return the error code
int gf2_fail_msg(const char *what);
int gf2_fail_hip(hipError_t e, const char *what);
// scratch from the per-stream arena of m4ri_hip_api.cpp (grown on demand, reused by later calls on the stream, released by
// gf2_trim); slots 0-3 belong to the products, 4 / 5 to gf2_trsm.hip (block inverses / a leaf's result)
int gf2_stream_scratch(hipStream_t s, size_t bytes, void **out, int slot);
// counts a run of a host routine of the size dispatch (gf2_host_small_calls)
void gf2_note_host_small_call();
// pooled device memory of m4ri_hip_api.cpp for the other translation units (gf2_nullspace.hip).  gf2_dev_free is not stream-ordered: the
// caller has synchronised every stream that touched the block
int gf2_dev_alloc(void **p, size_t bytes);
void gf2_dev_free(void *p, size_t bytes);
// the reduced row echelon form of gf2_echelonize_dev(full = 1, all columns) that also hands over the elimination's device array of pivot
// columns: *pivcols_dev (null when the matrix is empty) is released with gf2_dev_free(*pivcols_dev, *pivcols_bytes); pivcols_host may
// be null.  Synchronous on s.
int gf2_rref_keep_pivots_dev(gf2_dmat *A, int *rank, int *pivcols_host, void **pivcols_dev, size_t *pivcols_bytes, hipStream_t s);
// gf2_prof_enable's switch (gf2_nullspace.hip times its assembly launch while it is on)
bool gf2_prof_is_on();
