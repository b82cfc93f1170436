// runtime_host.cpp -- what every entry point of libm4ri_hip.so stands on: the error state, the launch census, pooled device memory,
// deferred frees, per-stream scratch arenas, streams, kernel timing, and gf2_dmat allocation / upload / download.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>

#include "api_internal.h"
#include "gf2_kernels.h"

typedef uint64_t u64;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------

static thread_local std::string tls_error;

int gf2_fail_hip(hipError_t e, const char *what) {
  tls_error = std::string(what) + ": " + hipGetErrorString(e);
  (void)hipGetLastError();
  return (int)e ? (int)e : -1;
}
int gf2_fail_msg(const char *what) {
  tls_error = what;
  return -1;
}

extern "C" const char *gf2_last_error(void) { return tls_error.c_str(); }

extern "C" int gf2_device_count(void) {
  static int n = [] {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
      (void)hipGetLastError();
      c = 0;
    }
    return c;
  }();
  return n;
}

int gf2_require_device() {
  if (gf2_device_count() <= 0)
    return gf2_fail_msg("no usable HIP device: libm4ri_hip has no CPU fallback for the multiply path");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// launch census: how often each kernel of the library has been launched by this process
// ---------------------------------------------------------------------------------------------

namespace {
// open-addressing table keyed by the kernel's host-side handle; lock-free (a launch pays a hash and one atomic increment)
struct CensusSlot {
  std::atomic<const void *> key{nullptr};
  std::atomic<unsigned long long> count{0};
};
constexpr unsigned kCensusSlots = 1024;  // the library has ~130 kernels
CensusSlot g_census[kCensusSlots];

std::string census_text() {
  std::string out;
  for (unsigned i = 0; i < kCensusSlots; ++i) {
    const void *k = g_census[i].key.load(std::memory_order_acquire);
    if (!k) continue;
    const char *nm = hipKernelNameRefByPtr(k, nullptr);
    out += std::to_string(g_census[i].count.load(std::memory_order_relaxed));
    out += ' ';
    out += nm ? nm : "?";
    out += '\n';
  }
  return out;
}

// M4RI_HIP_KERNEL_CENSUS_FILE=<path>: the counts of this process are APPENDED to the file when the library is unloaded (test suites
// that launch kernels from child processes: tests/conftest.py sets it for the whole session)
struct CensusDump {
  ~CensusDump() {
    const char *path = std::getenv("M4RI_HIP_KERNEL_CENSUS_FILE");
    if (!path || !*path) return;
    const std::string t = census_text();
    if (t.empty()) return;
    if (FILE *f = std::fopen(path, "a")) {
      std::fwrite(t.data(), 1, t.size(), f);
      std::fclose(f);
    }
  }
} g_census_dump;
}  // namespace

void gf2k_note_launch(const void *kernel) {
  unsigned i = (unsigned)((reinterpret_cast<uintptr_t>(kernel) >> 3) * 2654435761u) % kCensusSlots;
  for (unsigned probe = 0; probe < kCensusSlots; ++probe, i = (i + 1) % kCensusSlots) {
    const void *k = g_census[i].key.load(std::memory_order_acquire);
    if (k == kernel) break;
    if (!k) {
      const void *expect = nullptr;
      if (g_census[i].key.compare_exchange_strong(expect, kernel, std::memory_order_acq_rel) || expect == kernel) break;
    }
  }
  g_census[i].count.fetch_add(1, std::memory_order_relaxed);
}

// "<count> <mangled kernel name>\n" for every kernel launched so far; returns the length of the whole text (without the
// terminator), of which at most cap - 1 bytes are written to buf
extern "C" size_t gf2_kernel_census(char *buf, size_t cap) {
  const std::string t = census_text();
  if (buf && cap) {
    const size_t n = t.size() < cap - 1 ? t.size() : cap - 1;
    std::memcpy(buf, t.data(), n);
    buf[n] = 0;
  }
  return t.size();
}

// ---------------------------------------------------------------------------------------------
// device memory: small caching allocator (hipMalloc is slow and synchronising)
// ---------------------------------------------------------------------------------------------

namespace {
struct DevPool {
  std::mutex mu;
  std::multimap<size_t, void *> free_;
  size_t cached = 0;
};
DevPool g_pools[16];
// how gf2_dev_alloc served its requests so far: [0] from the block cache, [1] by a fresh hipMalloc (gf2_dev_alloc_counts)
std::atomic<long long> g_alloc_counts[2];

size_t round_size(size_t b) {
  const size_t g = b < ((size_t)64 << 20) ? ((size_t)1 << 20) : ((size_t)64 << 20);
  return ((b + g - 1) / g) * g;
}

// every block remembers the device it was allocated on: a free (possibly deferred, possibly issued while another device
// is current) files it under THAT device's pool
std::mutex g_owner_mu;
std::map<void *, int> g_owner;

void remember_owner(void *p, int dev) {
  std::lock_guard<std::mutex> lk(g_owner_mu);
  g_owner[p] = dev;
}
int owner_of(void *p, bool forget) {
  std::lock_guard<std::mutex> lk(g_owner_mu);
  auto it = g_owner.find(p);
  if (it == g_owner.end()) return -1;
  const int d = it->second;
  if (forget) g_owner.erase(it);
  return d;
}

// hipFree acts on the pointer's own device, but wants that device's context alive: keep the caller's device current
void raw_free(void *p) {
  (void)owner_of(p, true);
  (void)hipFree(p);
}

// deferred frees for asynchronous device-API calls: buffers used by work queued on a stream are
// handed back to the pool only after an event recorded behind that work has completed.
struct Deferred {
  hipEvent_t ev;
  void *p;
  size_t bytes;
};
std::mutex g_deferred_mu;
std::vector<Deferred> g_deferred;

// Per-stream scratch arena: work queued on one stream is serialised, so consecutive products on the same
// stream can share one workspace without waiting for each other.  It only ever grows.
struct StreamWs {
  void *p = nullptr;
  size_t bytes = 0;
};
std::mutex g_ws_mu;
std::map<std::tuple<int, hipStream_t, int>, StreamWs> g_ws;
}  // namespace

int gf2_dev_alloc(void **p, size_t bytes) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  bytes = round_size(bytes ? bytes : 1);
  DevPool &pool = g_pools[dev & 15];
  {
    std::lock_guard<std::mutex> lk(pool.mu);
    auto it = pool.free_.lower_bound(bytes);
    if (it != pool.free_.end() && it->first <= bytes + bytes / 4) {
      *p = it->second;
      pool.cached -= it->first;
      pool.free_.erase(it);
      g_alloc_counts[0].fetch_add(1, std::memory_order_relaxed);
      return 0;
    }
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    // drop the cache and retry once
    std::lock_guard<std::mutex> lk(pool.mu);
    for (auto &kv : pool.free_) raw_free(kv.second);
    pool.free_.clear();
    pool.cached = 0;
    (void)hipGetLastError();
    e = hipMalloc(p, bytes);
  }
  if (e != hipSuccess) return gf2_fail_hip(e, "hipMalloc");
  remember_owner(*p, dev);
  g_alloc_counts[1].fetch_add(1, std::memory_order_relaxed);
  return 0;
}

// out[0]: requests gf2_dev_alloc has served from the block cache, out[1]: by a fresh hipMalloc, since the library was loaded
extern "C" void gf2_dev_alloc_counts(long long out[2]) {
  out[0] = g_alloc_counts[0].load(std::memory_order_relaxed);
  out[1] = g_alloc_counts[1].load(std::memory_order_relaxed);
}

// Hands a block back to the pool of the device that owns it.  NOT stream-ordered: the caller guarantees that no queued
// work still touches the block (it synchronised its stream, or it goes through free_after / gf2_dmat_free).
void gf2_dev_free(void *p, size_t bytes) {
  if (!p) return;
  int dev = owner_of(p, false);
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return;
  bytes = round_size(bytes ? bytes : 1);
  DevPool &pool = g_pools[dev & 15];
  std::lock_guard<std::mutex> lk(pool.mu);
  static const size_t kMaxCached = (size_t)32 << 30;
  if (pool.cached + bytes > kMaxCached) {
    raw_free(p);
    return;
  }
  pool.free_.emplace(bytes, p);
  pool.cached += bytes;
}

// private per-thread streams of the host (mzd_t) entry points, one per device: concurrent calls from several host threads
// (BinMatrix is Send + Sync) never serialise on, or race through, a shared stream.  A thread that alternates between
// devices (a pinned multiply, then an elimination on the original device) gets the SAME stream back for each of them,
// so the per-stream arenas (g_ws) are reused instead of being stranded behind a replaced stream.
static thread_local hipStream_t tls_streams[16] = {};

int gf2_private_stream(hipStream_t *out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 16) return gf2_fail_msg("device ordinal out of range (0..15)");
  if (!tls_streams[dev]) HIP_TRY(hipStreamCreateWithFlags(&tls_streams[dev], hipStreamNonBlocking));
  *out = tls_streams[dev];
  return 0;
}

static void gf2_reap_deferred(bool wait) {
  std::lock_guard<std::mutex> lk(g_deferred_mu);
  size_t k = 0;
  for (size_t i = 0; i < g_deferred.size(); ++i) {
    Deferred &d = g_deferred[i];
    hipError_t q = wait ? hipEventSynchronize(d.ev) : hipEventQuery(d.ev);
    if (q == hipSuccess) {
      (void)hipEventDestroy(d.ev);
      gf2_dev_free(d.p, d.bytes);
    } else {
      (void)hipGetLastError();
      g_deferred[k++] = d;
    }
  }
  g_deferred.resize(k);
}

static int gf2_free_after(hipStream_t s, void *p, size_t bytes) {
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (hipError_t e = hipEventRecord(ev, s); e != hipSuccess) {  // e.g. a destroyed stream or one of another device
    (void)hipEventDestroy(ev);
    return gf2_fail_hip(e, "hipEventRecord");
  }
  std::lock_guard<std::mutex> lk(g_deferred_mu);
  g_deferred.push_back({ev, p, bytes});
  return 0;
}

int gf2_stream_scratch(hipStream_t s, size_t bytes, void **out, int slot) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_ws_mu);
  StreamWs &w = g_ws[std::make_tuple(dev, s, slot)];
  if (w.bytes < bytes) {
    if (w.p) {  // still referenced by queued work: hand it back once the stream has drained past this point
      if (gf2_free_after(s, w.p, w.bytes) != 0) {
        (void)hipStreamSynchronize(s);
        gf2_dev_free(w.p, w.bytes);
      }
      w.p = nullptr;
      w.bytes = 0;
    }
    gf2_reap_deferred(false);
    void *p = nullptr;
    if (int rc = gf2_dev_alloc(&p, bytes)) return rc;
    w.p = p;
    w.bytes = bytes;
  }
  *out = w.p;
  return 0;
}

// Give cached device memory back to the driver: waits for the device, then frees the per-stream scratch arenas (a
// 131072^3 product leaves a 141 GiB Strassen arena behind), the deferred frees and the block cache of the current
// device.  Safe at any quiet point; the next product allocates again.
extern "C" int gf2_trim(void) {
  if (int rc = gf2_require_device()) return rc;
  HIP_TRY(hipDeviceSynchronize());
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (auto it = g_ws.begin(); it != g_ws.end();) {
      if (std::get<0>(it->first) == dev) {
        gf2_dev_free(it->second.p, it->second.bytes);
        it = g_ws.erase(it);
      } else {
        ++it;
      }
    }
  }
  gf2_reap_deferred(true);
  DevPool &pool = g_pools[dev & 15];
  std::lock_guard<std::mutex> lk(pool.mu);
  for (auto &kv : pool.free_) raw_free(kv.second);
  pool.free_.clear();
  pool.cached = 0;
  return 0;
}

// Side streams + events for one main stream: the leaf products of a Strassen product run there, chunk by chunk, while
// the main stream streams the operands of the next chunk / folds the previous chunk's products (HBM-bound passes under
// an LDS-bound kernel).  Cached per (device, stream); never destroyed (a handful per process).
static std::map<std::pair<int, hipStream_t>, SideStream> g_side;

int gf2_side_stream(hipStream_t s, int nevents, SideStream **out, bool want_s3) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_ws_mu);
  SideStream &sd = g_side[{dev, s}];
  if (!sd.s2) HIP_TRY(hipStreamCreateWithFlags(&sd.s2, hipStreamNonBlocking));
  if (want_s3 && !sd.s3) HIP_TRY(hipStreamCreateWithFlags(&sd.s3, hipStreamNonBlocking));
  while ((int)sd.ev.size() < nevents) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    sd.ev.push_back(e);
  }
  *out = &sd;
  return 0;
}

// what the Strassen arena of a product on stream s may grow to (see api_internal.h)
size_t gf2_dev_arena_limit(hipStream_t s) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return SIZE_MAX;
  }
  size_t mine = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto it = g_ws.find(std::make_tuple(dev, s, (int)GF2_SLOT_OPERANDS));
    if (it != g_ws.end()) mine += it->second.bytes;
  }
  {
    DevPool &pool = g_pools[dev & 15];
    std::lock_guard<std::mutex> lk(pool.mu);
    mine += pool.cached;
  }
  return (size_t)((free_b + mine) * 0.95);
}

// ---------------------------------------------------------------------------------------------
// kernel timing (bench.py roofline): events around the dominant multiply kernel
// ---------------------------------------------------------------------------------------------

namespace {
std::mutex g_prof_mu;
bool g_prof_on = false;
struct ProfPair {
  hipEvent_t a, b;
};
std::vector<ProfPair> g_prof;

}  // namespace

extern "C" void gf2_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
}

bool gf2_prof_is_on() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  return g_prof_on;
}

extern "C" int gf2_prof_read(int *launches, double *ms, int reset) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double total = 0;
  for (auto &pp : g_prof) {
    HIP_TRY(hipEventSynchronize(pp.b));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, pp.a, pp.b));
    total += t;
  }
  if (launches) *launches = (int)g_prof.size();
  if (ms) *ms = total;
  if (reset) {
    for (auto &pp : g_prof) {
      (void)hipEventDestroy(pp.a);
      (void)hipEventDestroy(pp.b);
    }
    g_prof.clear();
  }
  return 0;
}

ProfScope::ProfScope(hipStream_t s_) : s(s_) {
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    on = g_prof_on;
  }
  if (on && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, s) != hipSuccess)) {
    (void)hipGetLastError();
    on = false;
  }
}
ProfScope::~ProfScope() {
  if (!on) return;
  if (hipEventRecord(b, s) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.push_back({a, b});
}

// ---------------------------------------------------------------------------------------------
// device matrices <-> host mzd_t
// ---------------------------------------------------------------------------------------------

extern "C" int gf2_dmat_alloc(gf2_dmat *M, int nrows, int ncols) {
  if (int rc = gf2_require_device()) return rc;
  if (!M || nrows < 0 || ncols < 0) return gf2_fail_msg("gf2_dmat_alloc: bad arguments");
  M->nrows = nrows;
  M->ncols = ncols;
  M->ld = dev_ld_for(ncols);
  void *p = nullptr;
  if (int rc = gf2_dev_alloc(&p, (size_t)(nrows ? nrows : 1) * M->ld * sizeof(u64))) return rc;
  M->data = static_cast<u64 *>(p);
  return 0;
}

// internal: the caller has already waited for every stream that touched M
void gf2_dmat_release(gf2_dmat *M) {
  if (!M || !M->data) return;
  gf2_dev_free(M->data, (size_t)(M->nrows ? M->nrows : 1) * M->ld * sizeof(u64));
  M->data = nullptr;
}

// Public free = hipFree semantics: the device API is asynchronous, so the block may still be read or written by queued
// work on any stream; wait for the owning device before the block can be handed to another caller.
extern "C" void gf2_dmat_free(gf2_dmat *M) {
  if (!M || !M->data) return;
  int cur = 0, own = owner_of(M->data, false);
  if (hipGetDevice(&cur) != hipSuccess) cur = -1;
  if (own >= 0 && cur >= 0 && own != cur) (void)hipSetDevice(own);
  if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
  if (own >= 0 && cur >= 0 && own != cur) (void)hipSetDevice(cur);
  gf2_dmat_release(M);
}

// Stream-ordered free: the block returns to the pool once everything queued on `stream` so far has completed.  For
// matrices that were only ever used on that one stream (temporaries of a chain of device products).
extern "C" int gf2_dmat_free_async(gf2_dmat *M, void *stream) {
  if (!M || !M->data) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t bytes = (size_t)(M->nrows ? M->nrows : 1) * M->ld * sizeof(u64);
  if (gf2_free_after(s, M->data, bytes) != 0) {  // could not record an event: fall back to waiting
    gf2_dmat_free(M);
    return 0;
  }
  M->data = nullptr;
  gf2_reap_deferred(false);
  return 0;
}

extern "C" int gf2_dmat_fill_random_block(gf2_dmat *M, uint64_t seed, int64_t row0, int64_t col_word0, int full_ncols,
                                          void *stream) {
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(gf2k_fill_random(M->data, M->ld, M->nrows, M->ncols, seed, row0, full_ncols > 0 ? (full_ncols + 63) >> 6 : 0,
                           col_word0, s));
  return 0;
}

extern "C" int gf2_dmat_fill_random_rows(gf2_dmat *M, uint64_t seed, int64_t row0, void *stream) {
  return gf2_dmat_fill_random_block(M, seed, row0, 0, 0, stream);
}

extern "C" int gf2_dmat_fill_random(gf2_dmat *M, uint64_t seed, void *stream) {
  return gf2_dmat_fill_random_rows(M, seed, 0, stream);
}

// host rows -> device. Our mzd_t are single-block with a constant rowstride (mzd_host.cpp), windows included, so rows
// [r0, r0 + dst->nrows) of `src` are one strided region starting at src->rows[r0].
// Asynchronous form (internal): `src` must stay untouched until the stream has passed the copy.
int gf2_upload_rows_async(gf2_dmat *dst, mzd_t const *src, int r0, hipStream_t s) {
  if (r0 < 0 || r0 + dst->nrows > src->nrows || dst->ncols != src->ncols) return gf2_fail_msg("gf2_dmat_upload: dimension mismatch");
  if (dst->nrows == 0 || src->ncols == 0) return 0;
  const size_t wbytes = (size_t)src->width * sizeof(word);
  if (dst->ld == src->rowstride)
    HIP_TRY(hipMemcpyAsync(dst->data, src->rows[r0], ((size_t)(dst->nrows - 1) * src->rowstride + src->width) * sizeof(word),
                           hipMemcpyHostToDevice, s));
  else
    HIP_TRY(hipMemcpy2DAsync(dst->data, (size_t)dst->ld * sizeof(u64), src->rows[r0], (size_t)src->rowstride * sizeof(word),
                             wbytes, dst->nrows, hipMemcpyHostToDevice, s));
  return 0;
}
static int upload_async(gf2_dmat *dst, mzd_t const *src, hipStream_t s) {
  if (dst->nrows != src->nrows) return gf2_fail_msg("gf2_dmat_upload: dimension mismatch");
  return gf2_upload_rows_async(dst, src, 0, s);
}

// public form: returns once the host rows have been consumed (the caller may free or modify `src` right away;
// pinned blocks make the copy itself truly asynchronous, so this has to wait for it)
extern "C" int gf2_dmat_upload(gf2_dmat *dst, mzd_t const *src, void *stream) {
  if (int rc = gf2_require_device()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = upload_async(dst, src, s)) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// device -> rows [r0, r0 + src->nrows) of a host matrix; returns when they are complete in host memory
int gf2_download_rows(mzd_t *dst, int r0, gf2_dmat const *src, hipStream_t s) {
  if (r0 < 0 || r0 + src->nrows > dst->nrows || dst->ncols != src->ncols) return gf2_fail_msg("gf2_dmat_download: dimension mismatch");
  const int nrows = src->nrows;
  if (nrows == 0 || dst->ncols == 0) return 0;
  const size_t wbytes = (size_t)dst->width * sizeof(word);
  const bool windowed = (dst->flags & mzd_flag_windowed_zerooffset) != 0;
  if (windowed && dst->high_bitmask != m4ri_ffff) {
    // the last word of each row is shared with the parent matrix: merge under the mask
    std::vector<word> tmp((size_t)nrows * dst->width);
    HIP_TRY(hipMemcpy2DAsync(tmp.data(), wbytes, src->data, (size_t)src->ld * sizeof(u64), wbytes, nrows,
                             hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (rci_t i = 0; i < nrows; ++i) {
      word *d = dst->rows[r0 + i];
      const word *t = tmp.data() + (size_t)i * dst->width;
      for (wi_t j = 0; j + 1 < dst->width; ++j) d[j] = t[j];
      d[dst->width - 1] = (d[dst->width - 1] & ~dst->high_bitmask) | (t[dst->width - 1] & dst->high_bitmask);
    }
    return 0;
  }
  if (!windowed && src->ld == dst->rowstride)
    HIP_TRY(hipMemcpyAsync(dst->rows[r0], src->data, ((size_t)(nrows - 1) * dst->rowstride + dst->width) * sizeof(word),
                           hipMemcpyDeviceToHost, s));
  else
    HIP_TRY(hipMemcpy2DAsync(dst->rows[r0], (size_t)dst->rowstride * sizeof(word), src->data,
                             (size_t)src->ld * sizeof(u64), wbytes, nrows, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gf2_dmat_download(mzd_t *dst, gf2_dmat const *src, void *stream) {
  if (int rc = gf2_require_device()) return rc;
  if (dst->nrows != src->nrows || dst->ncols != src->ncols) return gf2_fail_msg("gf2_dmat_download: dimension mismatch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return gf2_download_rows(dst, 0, src, s);
}
