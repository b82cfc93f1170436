// host_san_stubs.cpp -- what the five host units of the library (mzd_host, gf2_small_host, ple_host, trsm_host, nullspace_host) need
// from the rest of it, for the stand-alone sanitizer build of tests/test_host_sanitized.py.  There is no device: every device entry
// returns the failure code and counts the call, so a case that leaves the size dispatch of the host routines fails loudly (host_san.cpp
// checks the counter) instead of skipping silently.
#include "api_internal.h"

int g_stub_devices = 0;       // what gf2_device_count answers (host_san.cpp raises it for the pinned-pool check)
int g_stub_device_calls = 0;  // calls of device entries
int g_stub_pin_requests = 0;  // calls of hipHostMalloc

void gf2_cache_forget(mzd_t const *) {}
mzd_t *gf2_transpose_from_side_copy(mzd_t *, mzd_t const *) { return nullptr; }
int gf2_host_transpose_gpu(mzd_t *, mzd_t const *) { return ++g_stub_device_calls, -1; }

extern "C" {
int gf2_device_count(void) { return g_stub_devices; }
const char *gf2_last_error(void) { return "host_san: there is no device"; }
int gf2_dmat_alloc(gf2_dmat *, int, int) { return ++g_stub_device_calls, -1; }
void gf2_dmat_free(gf2_dmat *) {}
int gf2_dmat_upload(gf2_dmat *, mzd_t const *, void *) { return ++g_stub_device_calls, -1; }
int gf2_dmat_download(mzd_t *, gf2_dmat const *, void *) { return ++g_stub_device_calls, -1; }
int gf2_trsm_dev(gf2_dmat const *, gf2_dmat *, int, int, void *) { return ++g_stub_device_calls, -1; }
int gf2_ple_dev(gf2_dmat *, int, int *, int *, int *, void *) { return ++g_stub_device_calls, -1; }
int gf2_pluq_solve_left_dev(gf2_dmat const *, int, const int *, const int *, gf2_dmat *, int, int *, void *) { return ++g_stub_device_calls, -1; }
int gf2_apply_p_dev(gf2_dmat *, const int *, int, int, int, void *) { return ++g_stub_device_calls, -1; }
int gf2_nullspace_dev(gf2_dmat *, gf2_dmat *, int *, int *, void *) { return ++g_stub_device_calls, -1; }
// mzd_invert_naive eliminates through the drop-in entry; below the size dispatch that is the host routine
rci_t mzd_echelonize(mzd_t *A, int full) { return gf2_echelonize_host_small(A, full); }
hipError_t hipHostMalloc(void **p, size_t, unsigned int) {
  ++g_stub_pin_requests;
  *p = nullptr;
  return hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *) { return ++g_stub_device_calls, hipErrorInvalidValue; }
hipError_t hipGetLastError(void) { return hipSuccess; }
}
