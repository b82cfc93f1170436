// m4ri_hip_api.cpp -- C-ABI of libm4ri_hip.so: the multiply family of M4RI on the GPU.
//
// Entry points replace (paths relative to /root/reference):
//   mzd_mul_m4rm / mzd_addmul_m4rm   m4ri-sys/src/brilliantrussian.rs:210-224
//   mzd_mul / mzd_addmul             m4ri-sys/src/strassen.rs:8-31
//   mzd_mul_naive / mzd_addmul_naive / _mzd_mul_naive / _mzd_mul_va   m4ri-sys/src/mzd.rs:150-181
// Ownership and error behaviour follow the callers in m4ri-rust/src/friendly/binary_matrix.rs:
// C == NULL -> allocate (line 465), NULL return only on failure of the product (lines 467-469),
// dimension mismatch aborts like m4ri_die.
//
// There is no CPU fallback in this file: every product is a HIP kernel launch.  (The runtime under these entry points is runtime_host.cpp,
// the launch planner mul_plan_host.cpp, the products on device matrices mul_dev_host.cpp, the elimination entry points elim_host.cpp.)
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>

#include "api_internal.h"
#include "gf2_kernels.h"
#include "mul_plan.h"

typedef uint64_t u64;

// Operand cache: device copies of host matrices that the caller declared constant (gf2_mzd_cache_on_device).  A product
// whose A or B is cached skips that upload -- the drop-in path of repeated A*v with a fixed A (mul_slice,
// binary_matrix.rs:416-431) is otherwise bound by moving A over PCIe every call.
// Entries are keyed by the matrix' BLOCK (mzd_t::blocks, which windows share with their parent, mzd.rs:323-346): a library
// call that writes through a window therefore drops the parent's copy too.  An entry is handed out as a shared reference
// that a product holds until its stream has drained, so gf2_mzd_uncache from another thread never frees a copy in use.
struct CachedOperand {
  gf2_dmat d{};
  int dev = 0;
  int nrows = 0, ncols = 0, rowstride = 0;
  const word *row0 = nullptr;
  ~CachedOperand() {
    if (d.data) gf2_dev_free(d.data, (size_t)(d.nrows ? d.nrows : 1) * d.ld * sizeof(u64));
  }
};
namespace {
std::mutex g_cache_mu;
std::map<const void *, std::shared_ptr<CachedOperand>> g_cache;

// Result side copies: the PACKED TRANSPOSED form of a fresh thin product, kept on the host next to the product.  The friendly layer
// turns every `&A * &v` into mzd_mul_naive(NULL, A, v^T) followed by mzd_transpose(NULL, result) (binary_matrix.rs:416-431,
// :332-361, :528-542): in M4RI's layout the 2^20 x 1 result is one 64-bit word per row, 8 MiB for 128 KiB of bits, and gathering
// bit 0 of 2^20 words on the host cost 204 us of a 565-us call (profiles/r05_av_breakdown.txt).  The device has those bits in a
// register file anyway: a product into a library-allocated (NULL) destination with at most M4RI_HIP_RESULT_SIDE_COLS columns also
// transposes C on the device (one launch) and brings the n x m form down beside C; mzd_transpose of that matrix is then a copy.
// Keyed like the operand cache by the matrix' block and dropped by the same gf2_cache_forget calls (every library routine that
// writes a matrix, and mzd_free).  Stores through rows[] are invisible to the library, as for the operand cache: a caller that
// makes them (m4ri-sys's mzd_write_bit, BinMatrix::set_window) would read the old bits back from mzd_transpose.  So the side copy
// is OPT-IN (M4RI_HIP_RESULT_SIDE_COLS or gf2_set_result_side_cols; default 0 = off), for callers that promise gf2_mzd_uncache
// after such stores.
struct ResultSide {
  word *buf = nullptr;  // pinned; ncols rows of ld words
  size_t bytes = 0;
  size_t ld = 0;
  int nrows = 0, ncols = 0, rowstride = 0;  // of the product
  const word *row0 = nullptr;
  bool written = false;  // set by the paths that fill buf; a schedule that ignores the side copy leaves it unregistered
  ~ResultSide() { gf2_pinned_free(buf, bytes); }
};
std::map<const void *, std::shared_ptr<ResultSide>> g_result_side;
std::atomic<int> &result_side_cols() {
  static std::atomic<int> cols{env_int("M4RI_HIP_RESULT_SIDE_COLS", 0)};
  return cols;
}

static inline const void *cache_key(const mzd_t *M) { return M->blocks ? static_cast<const void *>(M->blocks) : M; }

}  // namespace

std::shared_ptr<CachedOperand> gf2_cache_lookup(const mzd_t *M) {
  std::lock_guard<std::mutex> lk(g_cache_mu);
  auto it = g_cache.find(cache_key(M));
  if (it == g_cache.end()) return nullptr;
  const CachedOperand &c = *it->second;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != c.dev) return nullptr;
  // the same view of the block (a window of a cached parent, or the parent of a cached window, is a different operand)
  if (c.nrows != M->nrows || c.ncols != M->ncols || c.rowstride != M->rowstride || (M->nrows && c.row0 != M->rows[0])) return nullptr;
  return it->second;
}

// device copy of rows [r0, r1) of M whose row stride equals the host row stride when the host block is contiguous, so
// that the transfer is one linear DMA
int gf2_to_device_rows(DMatOwner &o, const mzd_t *M, int r0, int r1, hipStream_t s, bool copy) {
  if (copy && r0 == 0 && r1 == M->nrows) {
    if (auto hit = gf2_cache_lookup(M)) {  // a read-only operand that already lives on the device
      o.d = hit->d;
      o.borrowed = std::move(hit);
      return 0;
    }
  }
  o.d.nrows = r1 - r0;
  o.d.ncols = M->ncols;
  const bool windowed = (M->flags & mzd_flag_windowed_zerooffset) != 0;
  o.d.ld = (!windowed && M->rowstride >= 1) ? M->rowstride : dev_ld_for(M->ncols);
  void *p = nullptr;
  if (int rc = gf2_dev_alloc(&p, (size_t)(o.d.nrows ? o.d.nrows : 1) * o.d.ld * sizeof(u64))) return rc;
  o.d.data = static_cast<u64 *>(p);
  if (copy) return gf2_upload_rows_async(&o.d, M, r0, s);  // the callers synchronise before they return
  return 0;
}
int gf2_to_device(DMatOwner &o, const mzd_t *M, hipStream_t s, bool copy) { return gf2_to_device_rows(o, M, 0, M->nrows, s, copy); }

// the ordinals of a comma-separated device list (M4RI_HIP_DEVICES), those that exist
static std::vector<int> parse_device_list(const char *e) {
  std::vector<int> out;
  const int nvis = gf2_device_count();
  for (const char *p = e; p && *p;) {
    char *end = nullptr;
    const long d = std::strtol(p, &end, 10);
    if (end == p) break;
    if (d >= 0 && d < nvis) out.push_back((int)d);
    p = (*end == ',') ? end + 1 : end;
    if (*end && *end != ',') break;
  }
  return out;
}

PinnedDevice::PinnedDevice() {
    const char *e = std::getenv("M4RI_HIP_DEVICES");
    if (!e || !*e || std::strcmp(e, "auto") == 0 || std::strcmp(e, "all") == 0) return;
    const std::vector<int> d = parse_device_list(e);
    if (d.size() != 1) return;
    if (hipGetDevice(&prev) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (prev != d[0] && hipSetDevice(d[0]) == hipSuccess) switched = true;
  }
PinnedDevice::~PinnedDevice() {
  if (switched) (void)hipSetDevice(prev);
}


namespace {
// Streams for the worker threads of a multi-device product: leased from a per-device pool for the duration of a call
// (a thread_local stream per short-lived worker would leak one stream, and its scratch arenas, per call).
std::mutex g_lease_mu;
std::vector<hipStream_t> g_lease[16];
int lease_stream(int dev, hipStream_t *out) {
  {
    std::lock_guard<std::mutex> lk(g_lease_mu);
    auto &v = g_lease[dev & 15];
    if (!v.empty()) {
      *out = v.back();
      v.pop_back();
      return 0;
    }
  }
  HIP_TRY(hipStreamCreateWithFlags(out, hipStreamNonBlocking));  // on the current device: the caller has set `dev`
  return 0;
}
void unlease_stream(int dev, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_lease_mu);
  g_lease[dev & 15].push_back(s);
}

// Rows [r0, r0 + c.nrows) of a fresh thin product C (r0 a multiple of 64) into their words of every row of the side copy.  The
// transposition kernel stores straight into the pinned host buffer (device-visible like every hipHostMalloc block; 128 KiB for
// 2^20 x 1): no scratch and no second download queued behind C's on the copy engine.  Complete once stream s has been synchronised.
int result_side_rows(ResultSide *side, const gf2_dmat &c, int r0, hipStream_t s) {
  const hipError_t e = gf2k_transpose(reinterpret_cast<u64 *>(side->buf) + r0 / 64, (long long)side->ld, c.data, c.ld, c.nrows, c.ncols, s);
  if (e != hipSuccess) return gf2_fail_hip(e, "gf2k_transpose");
  side->written = true;
  return 0;
}

// One to four vectors against many rows of 65..256 bits: the table-free kernel packs the side copy itself (a ballot per vector and 64
// rows), so product and transposed form are ONE launch.  1 = done, 0 = not this shape (the caller multiplies and transposes), < 0 error.
bool thin_vector_shape(int m, int l, int n) { return n >= 1 && n <= 4 && l > 64 && l <= 256 && m >= 262144; }
int thin_product_with_side(ResultSide *side, u64 *c, long long ldc, const u64 *a, long long lda, const gf2_dmat &b, int m, int l, hipStream_t s) {
  if (!side || !thin_vector_shape(m, l, b.ncols)) return 0;
  const hipError_t e = gf2k_tallskinny_side(a, lda, b.data, b.ld, c, ldc, m, l, b.ncols, reinterpret_cast<u64 *>(side->buf), (long long)side->ld, s);
  if (e == hipErrorNotSupported) return 0;
  if (e != hipSuccess) return gf2_fail_hip(e, "gf2k_tallskinny_side");
  side->written = true;
  return 1;
}

// One device's share of a host product: C[r0:r1, :] (+)= A[r0:r1, :] * B on the CURRENT device, stream s.  Four ways to run it,
// each a member function below; host_mul_range picks.
struct HostMulArgs {
  mzd_t *C;
  const mzd_t *A, *B;
  int r0, r1, accumulate, algo, param;
  hipStream_t s;
  ResultSide *side;  // not null: the product is fresh (library-allocated) and thin: leave its packed transposed form here
  int slabs(const HostPlan &hplan) const;
  int row_blocks(bool thin, int pipe_blocks) const;
  int plain() const;
  int zero_copy() const;
};

// (a) Slabs of the inner dimension: C (+)= A[G, K_s] B[K_s, :] for every row group G in turn (plan_host_product chose the slab lists); a
// finished group's rows of C leave while the next group is multiplied, the LAST group's last slab runs in four row blocks whose rows
// leave one by one.
int HostMulArgs::slabs(const HostPlan &hplan) const {
  const int rows = r1 - r0;
  int rc = 0;
  const int NR = (int)hplan.gslabs.size(), NBL = 4, RGr = rows / NR;
  int nslabs = 0;
  for (const auto &g : hplan.gslabs) nslabs += (int)g.size();
  SideStream *sd = nullptr;
  rc = gf2_side_stream(s, nslabs + NR + NBL, &sd, /*want_s3=*/true);
  DMatOwner dA, dB, dC;
  const bool bcached = (bool)gf2_cache_lookup(B);
  if (!rc) rc = gf2_to_device(dB, B, sd->s2, bcached);  // a cached B is borrowed (nothing is copied); otherwise allocated here, uploaded by slabs
  if (!rc) rc = gf2_to_device_rows(dA, A, r0, r1, s, false);
  if (!rc) rc = gf2_to_device_rows(dC, C, r0, r1, s, false);
  if (!rc && (dA.d.ld != A->rowstride || dC.d.ld != C->rowstride || (!bcached && dB.d.ld != B->rowstride)))
    rc = gf2_fail_msg("host pipeline: unexpected device stride");
  hipEvent_t *evU = sd ? sd->ev.data() : nullptr, *evC = evU + nslabs;
  auto rows_bytes = [](const mzd_t *M, int nr) { return ((size_t)(nr - 1) * M->rowstride + M->width) * sizeof(word); };
  for (int g = 0, ev = 0; !rc && g < NR; ++g) {  // every upload is queued at once: the next piece travels while this one is multiplied
    int k0 = 0;
    for (size_t si = 0; !rc && si < hplan.gslabs[g].size(); ++si, ++ev) {
      const int ks = hplan.gslabs[g][si];
      if (hipMemcpy2DAsync(dA.d.data + (size_t)g * RGr * dA.d.ld + k0 / 64, (size_t)dA.d.ld * sizeof(u64), A->rows[r0 + g * RGr] + k0 / 64,
                           (size_t)A->rowstride * sizeof(word), (size_t)ks / 8, (size_t)RGr, hipMemcpyHostToDevice, sd->s2) != hipSuccess ||
          (!bcached && g == 0 &&
           hipMemcpyAsync(dB.d.data + (size_t)k0 * dB.d.ld, B->rows[k0], rows_bytes(B, ks), hipMemcpyHostToDevice, sd->s2) != hipSuccess) ||
          hipEventRecord(evU[ev], sd->s2) != hipSuccess)
        rc = gf2_fail_hip(hipGetLastError(), "host pipeline: upload of a slab");
      k0 += ks;
    }
  }
  int nev_c = 0;
  auto download = [&](int row0, int nr, const gf2_dmat &c) {
    if (hipEventRecord(evC[nev_c], s) != hipSuccess || hipStreamWaitEvent(sd->s3, evC[nev_c], 0) != hipSuccess ||
        hipMemcpyAsync(C->rows[r0 + row0], c.data, rows_bytes(C, nr), hipMemcpyDeviceToHost, sd->s3) != hipSuccess)
      rc = gf2_fail_hip(hipGetLastError(), "host pipeline: download");
    ++nev_c;
  };
  for (int g = 0, ev = 0; !rc && g < NR; ++g) {
    int k0 = 0;
    const int S = (int)hplan.gslabs[g].size();
    for (int si = 0; !rc && si < S; ++si, ++ev) {
      const int ks = hplan.gslabs[g][si];
      if (hipStreamWaitEvent(s, evU[ev], 0) != hipSuccess) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: wait");
      gf2_dmat a = dA.d, b = dB.d, c = dC.d;
      a.data += (size_t)g * RGr * a.ld + k0 / 64;
      a.nrows = RGr;
      a.ncols = ks;
      b.data += (size_t)k0 * b.ld;
      b.nrows = ks;
      c.data += (size_t)g * RGr * c.ld;
      c.nrows = RGr;
      if (si + 1 < S || g + 1 < NR) {
        if (!rc) rc = gf2_mul_dispatch(&c, &a, &b, si > 0, algo, param, s, /*sync_free=*/false);
        if (!rc && si + 1 == S) download(g * RGr, RGr, c);
      } else {
        for (int bl = 0; !rc && bl < NBL; ++bl) {
          const int R = RGr / NBL;
          gf2_dmat ab = a, cb = c;
          ab.data += (size_t)bl * R * ab.ld;
          ab.nrows = R;
          cb.data += (size_t)bl * R * cb.ld;
          cb.nrows = R;
          rc = gf2_mul_dispatch(&cb, &ab, &b, si > 0, algo, param, s, /*sync_free=*/false);
          if (!rc) download(g * RGr + bl * R, R, cb);
        }
      }
      k0 += ks;
    }
  }
  if (sd && hipStreamSynchronize(sd->s2) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: upload stream");
  if (sd && sd->s3 && hipStreamSynchronize(sd->s3) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: download stream");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: compute stream");
  return rc;
}

// (b) Row blocks of A and C (contiguous rows) x halves of the inner dimension for the first block (contiguous rows of B):
//   C_i = A_i[:, 0:l/2] * B[0:l/2, :]  ^  A_i[:, l/2:l] * B[l/2:l, :]
// so that the first product can start after ONE block of A and HALF of B have arrived (7.3 ms of PCIe at n = 65536 instead of 12.2
// with all of B first) and every transfer is one linear copy.  Upload order: A_0, B top, B bottom, A_1, ...  `thin`: the LPN shapes,
// whose kernels stream A at HBM rate (the call IS the upload of A): two blocks, the second short.
int HostMulArgs::row_blocks(bool thin, int pipe_blocks) const {
  const int rows = r1 - r0;
  int rc = 0;
  const int l = A->ncols;
  const bool bcached = (bool)gf2_cache_lookup(B);
  const int K = (!bcached && l >= 8192 && l % 256 == 0 && B->rowstride >= 1 && !(B->flags & mzd_flag_windowed_zerooffset)) ? 2 : 1;
  SideStream *sd = nullptr;
  rc = gf2_side_stream(s, 2 * pipe_blocks + 3, &sd, /*want_s3=*/true);
  DMatOwner dA, dB, dC;
  if (!rc) rc = gf2_to_device(dB, B, sd->s2, K == 1);  // K == 2: allocated here, uploaded in halves below
  if (!rc) rc = gf2_to_device_rows(dA, A, r0, r1, s, false);
  if (!rc) rc = gf2_to_device_rows(dC, C, r0, r1, s, false);
  // block boundaries: four equal blocks, or -- when a quarter still has 16384 rows -- a quarter, a half and a quarter: the
  // half-size block multiplies at the rate of the big tiles (32768 x 32768 x 65536: 8.2 ms against 2 x 4.5 ms for two quarters)
  // while the first and the last block stay short (quick start, short tail of the download)
  std::vector<int> bnd;
  {
    const int q = rows / pipe_blocks;
    if (pipe_blocks == 4 && q >= 16384 && !thin) bnd = {0, q, 3 * q, rows};
    // a thin product is nothing but its copies: every block boundary costs ~20 us between two uploads, and what follows the last
    // upload (~100 us of fixed latencies: event -> kernel 26, kernel -> copy 35, the copies' own ~9 each) is exposed -- so two blocks,
    // the second short: 3/16 of the rows put the end of the first block's download where the second block's kernel ends
    // (2^20 x 256 x 1 under the profiler: 793 us with four equal blocks, 763 with these two; unpipelined 800; profiles/r05_av_timeline.txt)
    else if (thin && pipe_blocks == 4) bnd = {0, (int)((long long)rows * 13 / 16) & ~63, rows};
    else
      for (int i = 0; i <= pipe_blocks; ++i) bnd.push_back(i * q);
  }
  const int NBLK = (int)bnd.size() - 1;
  auto rows_bytes = [](const mzd_t *M, int nr) { return ((size_t)(nr - 1) * M->rowstride + M->width) * sizeof(word); };
  if (!rc && (dA.d.ld != A->rowstride || dC.d.ld != C->rowstride || (K == 2 && dB.d.ld != B->rowstride)))
    rc = gf2_fail_msg("host pipeline: unexpected device stride");
  hipEvent_t *evA = sd ? sd->ev.data() : nullptr, *evC = evA + pipe_blocks, *evB = evC + pipe_blocks;
  auto upload_a = [&](int i) {
    if (hipMemcpyAsync(dA.d.data + (size_t)bnd[i] * dA.d.ld, A->rows[r0 + bnd[i]], rows_bytes(A, bnd[i + 1] - bnd[i]), hipMemcpyHostToDevice,
                       sd->s2) != hipSuccess ||
        hipEventRecord(evA[i], sd->s2) != hipSuccess)
      rc = gf2_fail_hip(hipGetLastError(), "host pipeline: upload of A");
  };
  if (!rc) upload_a(0);
  for (int k = 0; !rc && k < K; ++k) {  // K == 1: B went up whole above (or lives in the operand cache)
    if (K == 2 && hipMemcpyAsync(dB.d.data + (size_t)k * (l / 2) * dB.d.ld, B->rows[k * (l / 2)], rows_bytes(B, l / 2), hipMemcpyHostToDevice,
                                 sd->s2) != hipSuccess)
      rc = gf2_fail_hip(hipGetLastError(), "host pipeline: upload of B");
    if (!rc && hipEventRecord(evB[k], sd->s2) != hipSuccess) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: event");
  }
  for (int i = 1; !rc && i < NBLK; ++i) upload_a(i);
  for (int i = 0; !rc && i < NBLK; ++i) {
    const int R = bnd[i + 1] - bnd[i];
    gf2_dmat c = dC.d;
    c.data += (size_t)bnd[i] * c.ld;
    c.nrows = R;
    if (hipStreamWaitEvent(s, evA[i], 0) != hipSuccess) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: wait");
    // only the FIRST block is multiplied in halves of the inner dimension (it starts while the bottom half of B is still on the
    // wire); by the time a later block has arrived all of B is resident, and one product over the whole inner dimension is the
    // more efficient launch (65536^3: 2 x 16384 x 32768 x 65536 take 9.2 ms, 16384 x 65536 x 65536 takes 8.2)
    const int Ki = i == 0 ? K : 1;
    for (int k = 0; !rc && k < Ki; ++k) {
      gf2_dmat a = dA.d, b = dB.d;
      a.data += (size_t)bnd[i] * a.ld + (size_t)k * (l / Ki) / 64;
      a.nrows = R;
      a.ncols = l / Ki;
      b.data += (size_t)k * (l / Ki) * b.ld;
      b.nrows = l / Ki;
      for (int kk = (Ki == 1 ? 0 : k); !rc && kk < (Ki == 1 ? K : k + 1); ++kk)
        if (hipStreamWaitEvent(s, evB[kk], 0) != hipSuccess) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: wait");
      if (!rc) rc = gf2_mul_dispatch(&c, &a, &b, k > 0, algo, param, s, /*sync_free=*/false);
    }
    if (!rc && (hipEventRecord(evC[i], s) != hipSuccess || hipStreamWaitEvent(sd->s3, evC[i], 0) != hipSuccess ||
                hipMemcpyAsync(C->rows[r0 + bnd[i]], c.data, rows_bytes(C, R), hipMemcpyDeviceToHost, sd->s3) != hipSuccess))
      rc = gf2_fail_hip(hipGetLastError(), "host pipeline: download");
    if (!rc && side) rc = result_side_rows(side, c, bnd[i], s);  // beside the block's download
  }
  if (sd && hipStreamSynchronize(sd->s2) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: upload stream");
  if (sd && sd->s3 && hipStreamSynchronize(sd->s3) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: download stream");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "host pipeline: compute stream");
  return rc;
}

// (c) Everything up, one product, everything down (small products, windows, accumulating calls, operands the pipelines do not take).
int HostMulArgs::plain() const {
  const int rows = r1 - r0;
  int rc = 0;
  DMatOwner dA, dB, dC;
  rc = gf2_to_device_rows(dA, A, r0, r1, s, true);
  if (!rc) rc = gf2_to_device(dB, B, s, true);
  if (!rc) rc = gf2_to_device_rows(dC, C, r0, r1, s, accumulate != 0);
  // (thin products: no wait between the kernel and the download -- the download's own launch latency would be exposed behind it)
  int fused = 0;  // product and side copy in one launch (one to four vectors)
  if (!rc && side && !accumulate) {
    fused = thin_product_with_side(side, dC.d.data, dC.d.ld, dA.d.data, dA.d.ld, dB.d, rows, A->ncols, s);
    if (fused < 0) rc = fused;
  }
  if (!rc && fused != 1) rc = gf2_mul_dispatch(&dC.d, &dA.d, &dB.d, accumulate, algo, param, s, /*sync_free=*/!(side || B->ncols <= 64));
  if (!rc && side && fused == 1) {
    rc = gf2_download_rows(C, r0, &dC.d, s);  // (syncs: the side copy is complete with it)
  } else if (!rc && side) {
    // C comes down on the download stream while the compute stream transposes it and brings the small form down
    SideStream *sd = nullptr;
    rc = gf2_side_stream(s, 1, &sd, /*want_s3=*/true);
    if (!rc && (hipEventRecord(sd->ev[0], s) != hipSuccess || hipStreamWaitEvent(sd->s3, sd->ev[0], 0) != hipSuccess ||
                hipMemcpyAsync(C->rows[r0], dC.d.data, ((size_t)(rows - 1) * C->rowstride + C->width) * sizeof(word), hipMemcpyDeviceToHost,
                               sd->s3) != hipSuccess))
      rc = gf2_fail_hip(hipGetLastError(), "thin product: download");
    if (!rc) rc = result_side_rows(side, dC.d, 0, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "thin product: compute stream");
    if (sd && sd->s3 && hipStreamSynchronize(sd->s3) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "thin product: download stream");
  } else if (!rc) rc = gf2_download_rows(C, r0, &dC.d, s);
  if (rc) (void)hipStreamSynchronize(s);
  return rc;
}

// (d) `&A * &v` with A on the host (round 5): the vector kernel reads A from, and writes C and the side copy into, the PINNED host
// blocks themselves -- the launch IS the transfer (32 MiB in at the rate a kernel pulls over PCIe, 8 MiB out beside it), with no copy
// queue between its pieces: 2^20 x 256 x 1 0.69 ms for the product against 0.77 through uploads, kernel and downloads in two row
// blocks (profiles/r05_zero_copy_probe.txt; the side copy is what made it worth having: it used to need C on the device).
// 1 = done, 0 = not this case, < 0 error.
int HostMulArgs::zero_copy() const {
  const int rows = r1 - r0;
  int rc = 0;
  DMatOwner dB;
  rc = gf2_to_device(dB, B, s, true);
  int done = 0;
  if (!rc) done = thin_product_with_side(side, C->rows[0], C->rowstride, A->rows[0], A->rowstride, dB.d, rows, A->ncols, s);
  if (done < 0) rc = done;
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "thin product: stream");
  return rc ? rc : done;
}

// Returns when rows [r0, r1) of C are complete in host memory.
int host_mul_range(mzd_t *C, const mzd_t *A, const mzd_t *B, int r0, int r1, int accumulate, int algo, int param, hipStream_t s,
                   ResultSide *side = nullptr) {
  const int rows = r1 - r0;
  if (rows <= 0) return 0;
  const HostMulArgs h{C, A, B, r0, r1, accumulate, algo, param, s, side};
  // Large products are pipelined: an upload stream brings the operands in, a download stream takes C out (PCIe is full duplex: the two
  // directions get a stream each), the compute stream multiplies a piece as soon as it has arrived -- PCIe is most of a host call:
  // 1.5 GiB at n = 65536.
  static const int pipe_blocks = env_int("M4RI_HIP_HOST_PIPELINE_BLOCKS", 4);  // (2 blocks at 32768 / 16384 rows measured slower: 9.7 / 2.1 against 9.0 / 1.9 ms)
  const bool plain_layout = !(A->flags & mzd_flag_windowed_zerooffset) && !(C->flags & mzd_flag_windowed_zerooffset) &&
                            A->rowstride >= 1 && C->rowstride >= 1;
  const bool whole = r0 == 0 && r1 == A->nrows;
  // (Round 4 measured a 2 x 2 plan for mid-sized products -- the four quadrants of C as units, A in two row blocks, B in two
  // column panels by 2-D copies, upload order A_0, B_0, B_1, A_1 -- against the row blocks at 32768^3: 8.6 against 8.8 ms.
  // The 2-D copies run at the linear rate (hipMemcpy2DAsync, 2 KiB rows: 54 GB/s), but a 16384 x 32768 x 16384 quadrant takes
  // 1.33-1.40 ms -- 49 leaves = 392 tiles = 1.5 rounds, run as a whole round plus a tail launch -- where a quarter of the whole
  // product's time would be 1.1: four of them are 5.5 ms of device work behind the 2.4 ms the first two pieces take to arrive.
  // Not kept: profiles/r04_host_path_timeline.txt.)
  static const int zero_copy = dev_env_int("M4RI_HIP_THIN_ZERO_COPY", 1);
  if (zero_copy && side && whole && !accumulate && plain_layout && thin_vector_shape(rows, A->ncols, B->ncols) && !gf2_cache_lookup(A) &&
      gf2_mzd_block_is_pinned(A) && gf2_mzd_block_is_pinned(C) && (size_t)rows * A->rowstride * sizeof(word) >= ((size_t)8 << 20)) {
    const int done = h.zero_copy();
    if (done != 0) return done < 0 ? done : 0;
  }
  // thin products (the LPN shape, 2^20 x 256 times a few vectors) are pipelined too
  const bool thin = B->ncols <= 256 && A->ncols <= 1024 && (size_t)rows * A->rowstride * sizeof(word) >= ((size_t)8 << 20);
  const bool pipelined = pipe_blocks >= 2 && !accumulate && plain_layout && rows >= 16384 && rows % (pipe_blocks * 64) == 0 &&
                         !(whole && gf2_cache_lookup(A));
  const bool big = (long long)A->ncols * B->ncols >= (1ll << 28);
  if (pipelined && big && pipe_blocks == 4 && B->rowstride >= 1 && !(B->flags & mzd_flag_windowed_zerooffset)) {
    const HostPlan hplan = plan_host_product(rows, A->ncols, B->ncols, algo, param, (bool)gf2_cache_lookup(B), (size_t)A->rowstride * sizeof(word),
                                             (size_t)B->rowstride * sizeof(word), (size_t)C->rowstride * sizeof(word));
    if (!hplan.gslabs.empty()) return h.slabs(hplan);
  }
  if (pipelined && (big || thin)) return h.row_blocks(thin, pipe_blocks);
  return h.plain();
}

// Devices a host product of this shape is spread over.  M4RI_HIP_DEVICES: unset = the current device only (the fan-out is
// opt-in: it has not been measured on a multi-GPU box yet, and under torchrun every rank sees every GPU); "auto" = every
// visible device once the product is large enough to pay for a copy of B per device -- ignored inside a torch.distributed
// job (WORLD_SIZE > 1), where the ranks already own a device each; "all"; or a comma-separated list of device ordinals
// (an ordinal may repeat: two shares on one device -- how the one-GPU test box exercises this path; ONE ordinal pins every
// host entry point -- products, elimination, transpose, operand cache -- to that device).
std::vector<int> pick_devices(long long m, long long l, long long n) {
  const char *e = std::getenv("M4RI_HIP_DEVICES");
  std::vector<int> out;
  if (!e || !*e) return out;
  const int nvis = gf2_device_count();
  const bool autom = std::strcmp(e, "auto") == 0, all = std::strcmp(e, "all") == 0;
  if (!autom && !all) return parse_device_list(e);
  if (autom) {
    const char *ws = std::getenv("WORLD_SIZE");
    if (ws && std::atoi(ws) > 1) return out;  // one process per GPU already
  }
  // automatic: a share should keep >= 4096 rows (tall tiles) and the product should outweigh moving B once more per device
  if (nvis > 1 && (all || (2.0 * (double)m * (double)l * (double)n >= 7.0e13 && m >= 8192))) {
    int k = nvis;
    while (k > 1 && m / k < 4096 && !all) --k;
    for (int d = 0; d < k; ++d) out.push_back(d);
  }
  return out;
}

// C (+)= A*B with the rows of A and C divided among `devs` (one worker thread per share; each uploads its rows of A and
// its own copy of B over its own PCIe link, multiplies, and downloads its rows of C).  Shares are independent: the inner
// dimension is never split, so there is no reduction.
int host_mul_multi(mzd_t *C, const mzd_t *A, const mzd_t *B, int accumulate, int algo, int param, const std::vector<int> &devs) {
  const int k = (int)devs.size(), m = A->nrows;
  // shares: equal, rounded up to a multiple of 1024 rows (whole tiles / Strassen-divisible blocks), the last one takes the rest
  long long per = ((long long)m + k - 1) / k;
  per = (per + 1023) / 1024 * 1024;
  std::vector<int> rcs(k, 0);
  std::vector<std::string> errs(k);
  std::vector<std::thread> th;
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (int t = 0; t < k; ++t) {
    const int r0 = (int)std::min<long long>(m, per * t), r1 = (int)std::min<long long>(m, per * (t + 1));
    if (r1 <= r0) continue;
    th.emplace_back([&, t, r0, r1] {
      const int dev = devs[t];
      if (hipSetDevice(dev) != hipSuccess) {
        rcs[t] = gf2_fail_hip(hipGetLastError(), "hipSetDevice");
        errs[t] = gf2_last_error();
        return;
      }
      hipStream_t s = nullptr;
      rcs[t] = lease_stream(dev, &s);
      if (!rcs[t]) {
        rcs[t] = host_mul_range(C, A, B, r0, r1, accumulate, algo, param, s);
        if (rcs[t]) (void)hipStreamSynchronize(s);
        unlease_stream(dev, s);
      }
      if (rcs[t]) errs[t] = gf2_last_error();
    });
  }
  for (auto &x : th) x.join();
  (void)hipSetDevice(cur);
  for (int t = 0; t < k; ++t)
    if (rcs[t]) {
      (void)gf2_fail_msg(("device " + std::to_string(devs[t]) + ": " + errs[t]).c_str());
      return rcs[t];
    }
  return 0;
}

mzd_t *host_mul_on(mzd_t *C, const mzd_t *A, const mzd_t *B, int accumulate, int algo, int param, const char *name,
                   const int *devices, int ndev) {
  if (A->ncols != B->nrows) gf2_die((std::string(name) + ": A ncols need to match B nrows.").c_str());
  if (accumulate && !C) gf2_die((std::string(name) + ": C must not be NULL.").c_str());
  const bool allocated = (C == nullptr);
  if (C && (C->nrows != A->nrows || C->ncols != B->ncols))
    gf2_die((std::string(name) + ": C (ret) has wrong dimensions.").c_str());
  auto bail = [&](const char *why) -> mzd_t * {
    std::fprintf(stderr, "m4ri_hip: %s failed: %s (%s)\n", name, why, gf2_last_error());
    return nullptr;
  };
  if (gf2_require_device()) return bail("no device");
  // size dispatch: a product of a few thousand word operations is done on the host by the time a
  // device call would have uploaded its operands (gf2_small_host.cpp); operands the caller pinned to the device stay there
  const bool small = !devices && gf2_small_product(A->nrows, A->ncols, B->ncols) && !gf2_cache_lookup(A) && !gf2_cache_lookup(B);
  if (!C) C = (small || A->nrows == 0 || B->ncols == 0) ? mzd_init(A->nrows, B->ncols) : gf2_mzd_init_uncleared(A->nrows, B->ncols);
  else gf2_cache_forget(C);  // about to be overwritten
  if (A->nrows == 0 || B->ncols == 0) return C;
  if (small) {
    if (gf2_mul_host_small(C, A, B, accumulate) == 0) return C;
    if (allocated) mzd_free(C);
    return bail("host product");
  }
  std::vector<int> devs;
  if (devices) {
    for (int i = 0; i < ndev; ++i) {
      if (devices[i] < 0 || devices[i] >= gf2_device_count()) {
        if (allocated) mzd_free(C);
        gf2_fail_msg("device ordinal out of range");
        return bail("device list");
      }
      devs.push_back(devices[i]);
    }
  } else {
    devs = pick_devices(A->nrows, A->ncols, B->ncols);
  }
  const bool windows = ((A->flags | C->flags) & mzd_flag_windowed_zerooffset) != 0;
  int rc;
  if (devs.size() > 1 && !windows) {
    rc = host_mul_multi(C, A, B, accumulate, algo, param, devs);
  } else {
    int cur = 0, want = devs.size() == 1 ? devs[0] : -1;
    if (want >= 0 && (hipGetDevice(&cur) != hipSuccess || hipSetDevice(want) != hipSuccess)) want = -1;
    hipStream_t s;
    if (gf2_private_stream(&s)) {
      if (allocated) mzd_free(C);
      return bail("stream");
    }
    // opted in: a fresh thin product also comes back in its packed transposed form (see ResultSide)
    const int side_cols = result_side_cols().load(std::memory_order_relaxed);
    std::shared_ptr<ResultSide> side;
    if (allocated && !windows && C->ncols <= side_cols && C->blocks && C->blocks[0].size >= ((size_t)1 << 20)) {
      side = std::make_shared<ResultSide>();
      side->ld = ((size_t)C->nrows + 63) / 64;
      side->bytes = (size_t)C->ncols * side->ld * sizeof(word);
      side->buf = static_cast<word *>(gf2_pinned_alloc(side->bytes));
      if (!side->buf) side.reset();  // pinning failed: the product does not depend on it
    }
    rc = host_mul_range(C, A, B, 0, A->nrows, accumulate, algo, param, s, side.get());
    if (want >= 0) (void)hipSetDevice(cur);
    if (!rc && side && side->written) {  // (the slab schedule does not write it)
      side->nrows = C->nrows;
      side->ncols = C->ncols;
      side->rowstride = C->rowstride;
      side->row0 = C->rows[0];
      std::lock_guard<std::mutex> lk(g_cache_mu);
      g_result_side[cache_key(C)] = std::move(side);
    }
  }
  if (rc) {
    if (allocated) mzd_free(C);
    return bail("device product");
  }
  return C;
}

mzd_t *host_mul(mzd_t *C, const mzd_t *A, const mzd_t *B, int accumulate, int algo, int param, const char *name) {
  return host_mul_on(C, A, B, accumulate, algo, param, name, nullptr, 0);
}
}  // namespace

// One process, several devices: C = A*B (C NULL: allocated) with the rows of A and C divided among `devices` (ordinals of
// hipGetDeviceCount's numbering; an ordinal may repeat).  mzd_mul / mzd_mul_m4rm / mzd_mul_naive do the same by
// themselves for large products when more than one device is visible (M4RI_HIP_DEVICES).
extern "C" mzd_t *gf2_mul_multi(mzd_t *C, mzd_t const *A, mzd_t const *B, int algo, int param, const int *devices, int ndev) {
  if (!A || !B || !devices || ndev < 1) {
    gf2_fail_msg("gf2_mul_multi: bad arguments");
    return nullptr;
  }
  return host_mul_on(C, A, B, 0, algo, param, "gf2_mul_multi", devices, ndev);
}

extern "C" int gf2_set_result_side_cols(int cols) { return result_side_cols().exchange(cols > 0 ? cols : 0); }

void gf2_cache_forget(mzd_t const *M) {
  std::shared_ptr<CachedOperand> c;
  std::shared_ptr<ResultSide> sd;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (!g_result_side.empty()) {
      auto it = g_result_side.find(cache_key(M));
      if (it != g_result_side.end()) {
        sd = std::move(it->second);
        g_result_side.erase(it);
      }
    }
    if (g_cache.empty()) return;
    auto it = g_cache.find(cache_key(M));
    if (it == g_cache.end()) return;
    c = std::move(it->second);
    g_cache.erase(it);
  }
  // products that looked the copy up hold their own reference until their stream has drained; the block goes back to the
  // pool when the last reference is dropped (here, if nobody is using it)
}

extern "C" int gf2_mzd_cache_on_device(mzd_t const *M) {
  if (int rc = gf2_require_device()) return rc;
  if (!M || M->nrows == 0 || M->ncols == 0) return gf2_fail_msg("gf2_mzd_cache_on_device: empty matrix");
  gf2_cache_forget(M);
  PinnedDevice pin;  // M4RI_HIP_DEVICES = one ordinal: run there
  hipStream_t s;
  if (int rc = gf2_private_stream(&s)) return rc;
  DMatOwner o;
  if (int rc = gf2_to_device(o, M, s, true)) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  auto c = std::make_shared<CachedOperand>();
  HIP_TRY(hipGetDevice(&c->dev));
  c->d = o.d;
  c->nrows = M->nrows;
  c->ncols = M->ncols;
  c->rowstride = M->rowstride;
  c->row0 = M->rows[0];
  o.released = true;  // ownership moves to the cache
  std::lock_guard<std::mutex> lk(g_cache_mu);
  g_cache[cache_key(M)] = std::move(c);
  return 0;
}

extern "C" void gf2_mzd_uncache(mzd_t const *M) { gf2_cache_forget(M); }

// mzd_transpose(DST, A) from the side copy of A, if A is a fresh thin product that still has one: DST (allocated when NULL) or nullptr.
mzd_t *gf2_transpose_from_side_copy(mzd_t *DST, mzd_t const *A) {
  std::shared_ptr<ResultSide> sd;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (g_result_side.empty()) return nullptr;
    auto it = g_result_side.find(cache_key(A));
    if (it == g_result_side.end()) return nullptr;
    sd = it->second;
  }
  // the same view of the block (a window of the product is a different matrix)
  if (sd->nrows != A->nrows || sd->ncols != A->ncols || sd->rowstride != A->rowstride || sd->row0 != A->rows[0] ||
      (A->flags & mzd_flag_windowed_zerooffset))
    return nullptr;
  const bool fresh = DST == nullptr;
  if (fresh) DST = gf2_mzd_init_uncleared(A->ncols, A->nrows);
  const wi_t w = DST->width;
  for (rci_t i = 0; i < DST->nrows; ++i) {
    word *d = DST->rows[i];
    const word *t = sd->buf + (size_t)i * sd->ld;
    if (w > 1) std::memcpy(d, t, (size_t)(w - 1) * sizeof(word));
    d[w - 1] = fresh ? (t[w - 1] & DST->high_bitmask) : ((d[w - 1] & ~DST->high_bitmask) | (t[w - 1] & DST->high_bitmask));
  }
  return DST;
}

int gf2_host_transpose_gpu(mzd_t *dst, mzd_t const *src) {
  if (gf2_require_device()) return -1;
  PinnedDevice pin;  // M4RI_HIP_DEVICES = one ordinal: run there
  hipStream_t s;
  if (gf2_private_stream(&s)) return -1;
  DMatOwner dS, dD;
  int rc = 0;
  // Large matrices in four or eight row blocks of the source: block i goes up on one copy stream, is transposed into ITS words of every row
  // of the destination, and those words come down through a 2-D copy on the other copy stream while block i + 1 goes up (PCIe is
  // full duplex; 2-D copies of 2-KiB pieces run at the linear rate, see host_mul_range).  65536^2: 19.3 -> 12.3 ms (9.4 ms per direction).
  static const int pipe_on = dev_env_int("M4RI_HIP_TRANSPOSE_PIPELINE", 1);  // 0 off, 1 by rule, n >= 2: n blocks (A/B)
  // (65536^2 on one box: 2 / 4 / 8 / 16 blocks 15.1 / 13.2 / 12.3 / 16.7 ms, unpipelined 19.3; 32768 x 65536: 4 blocks 6.6, 8 blocks 8.3 --
  // the 2-D copy wants pieces of at least 1 KiB)
  const int NB = pipe_on >= 2 ? pipe_on : (src->nrows >= 65536 ? 8 : 4);
  const bool plain = !(src->flags & mzd_flag_windowed_zerooffset) && !(dst->flags & mzd_flag_windowed_zerooffset) &&
                     src->rowstride >= 1 && dst->rowstride >= 1 && src->nrows > 0 && src->ncols > 0 &&
                     src->rows[src->nrows - 1] == src->rows[0] + (size_t)(src->nrows - 1) * src->rowstride &&
                     dst->rows[dst->nrows - 1] == dst->rows[0] + (size_t)(dst->nrows - 1) * dst->rowstride;
  if (pipe_on && plain && src->nrows % (NB * 512) == 0 && src->nrows / NB >= (pipe_on >= 2 ? 2048 : 8192) /* pieces of >= 1 KiB in the 2-D copies */ &&
      (long long)src->nrows * src->ncols >= (1ll << 31) && !gf2_cache_lookup(src)) {
    SideStream *side = nullptr;
    rc = gf2_side_stream(s, 2 * NB, &side, /*want_s3=*/true);
    if (!rc) rc = gf2_to_device(dS, src, s, false);
    if (!rc) rc = gf2_to_device(dD, dst, s, false);
    if (!rc && (dS.d.ld != src->rowstride || dD.d.ld != dst->rowstride)) rc = gf2_fail_msg("transpose pipeline: unexpected device stride");
    const int R = src->nrows / NB;
    hipEvent_t *evU = side ? side->ev.data() : nullptr, *evT = evU + NB;
    for (int i = 0; !rc && i < NB; ++i) {
      const size_t up = ((size_t)(R - 1) * src->rowstride + src->width) * sizeof(word);
      if (hipMemcpyAsync(dS.d.data + (size_t)i * R * dS.d.ld, src->rows[(size_t)i * R], up, hipMemcpyHostToDevice, side->s2) != hipSuccess ||
          hipEventRecord(evU[i], side->s2) != hipSuccess || hipStreamWaitEvent(s, evU[i], 0) != hipSuccess) {
        rc = gf2_fail_hip(hipGetLastError(), "transpose pipeline: upload");
        break;
      }
      const hipError_t e = gf2k_transpose(dD.d.data + (size_t)i * R / 64, dD.d.ld, dS.d.data + (size_t)i * R * dS.d.ld, dS.d.ld, R, src->ncols, s);
      if (e != hipSuccess) {
        rc = gf2_fail_hip(e, "gf2k_transpose");
        break;
      }
      if (hipEventRecord(evT[i], s) != hipSuccess || hipStreamWaitEvent(side->s3, evT[i], 0) != hipSuccess ||
          hipMemcpy2DAsync(dst->rows[0] + (size_t)i * R / 64, (size_t)dst->rowstride * sizeof(word), dD.d.data + (size_t)i * R / 64,
                           (size_t)dD.d.ld * sizeof(u64), (size_t)R / 8, (size_t)dst->nrows, hipMemcpyDeviceToHost, side->s3) != hipSuccess)
        rc = gf2_fail_hip(hipGetLastError(), "transpose pipeline: download");
    }
    if (side && hipStreamSynchronize(side->s2) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "transpose pipeline: upload stream");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "transpose pipeline: compute stream");
    if (side && side->s3 && hipStreamSynchronize(side->s3) != hipSuccess && !rc) rc = gf2_fail_hip(hipGetLastError(), "transpose pipeline: download stream");
    return rc;
  }
  rc = gf2_to_device(dS, src, s, true);
  if (!rc) rc = gf2_to_device(dD, dst, s, false);
  if (!rc) {
    hipError_t e = gf2k_transpose(dD.d.data, dD.d.ld, dS.d.data, dS.d.ld, src->nrows, src->ncols, s);
    if (e != hipSuccess) rc = gf2_fail_hip(e, "gf2k_transpose");
  }
  if (!rc) rc = gf2_dmat_download(dst, &dD.d, s);
  if (rc) (void)hipStreamSynchronize(s);
  return rc;
}

// Strassen levels from M4RI's cutoff argument: recursion continues while the halved dimension stays
// >= cutoff (strassen.rs:8-18: "Minimal dimension for Strassen recursion"); 0 = library default.
static int levels_from_cutoff(const mzd_t *A, const mzd_t *B, int cutoff) {
  if (cutoff <= 0) return 0;  // automatic
  const int mn = A->nrows < A->ncols ? (A->nrows < B->ncols ? A->nrows : B->ncols)
                                     : (A->ncols < B->ncols ? A->ncols : B->ncols);
  int L = 0;
  while (L < 6 && (mn >> (L + 1)) >= cutoff) ++L;
  return L ? L : -1;  // -1: explicit "no recursion"
}

extern "C" mzd_t *mzd_mul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k) {
  (void)k;  // table size hint; the kernel's tables are fixed at 8 bits (LDS bank-row geometry)
  return host_mul(C, A, B, 0, GF2_ALGO_M4RM, 0, "mzd_mul_m4rm");
}
extern "C" mzd_t *mzd_addmul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k) {
  (void)k;
  return host_mul(C, A, B, 1, GF2_ALGO_M4RM, 0, "mzd_addmul_m4rm");
}
extern "C" mzd_t *mzd_mul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) {
  const int L = levels_from_cutoff(A, B, cutoff);
  if (L < 0) return host_mul(C, A, B, 0, GF2_ALGO_M4RM, 0, "mzd_mul");
  return host_mul(C, A, B, 0, GF2_ALGO_STRASSEN, L, "mzd_mul");
}
extern "C" mzd_t *mzd_addmul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff) {
  const int L = levels_from_cutoff(A, B, cutoff);
  if (L < 0) return host_mul(C, A, B, 1, GF2_ALGO_M4RM, 0, "mzd_addmul");
  return host_mul(C, A, B, 1, GF2_ALGO_STRASSEN, L, "mzd_addmul");
}
extern "C" mzd_t *mzd_mul_naive(mzd_t *C, mzd_t const *A, mzd_t const *B) {
  return host_mul(C, A, B, 0, GF2_ALGO_NAIVE, 0, "mzd_mul_naive");
}
extern "C" mzd_t *mzd_addmul_naive(mzd_t *C, mzd_t const *A, mzd_t const *B) {
  return host_mul(C, A, B, 1, GF2_ALGO_NAIVE, 0, "mzd_addmul_naive");
}

extern "C" mzd_t *_mzd_mul_naive(mzd_t *C, mzd_t const *A, mzd_t const *Bt, int clear) {
  // C (+)= A * Bt^T, Bt pre-transposed (mzd.rs:154-168); C is "preallocated" upstream
  if (!C) gf2_die("_mzd_mul_naive: C must be preallocated.");
  if (A->ncols != Bt->ncols || C->nrows != A->nrows || C->ncols != Bt->nrows)
    gf2_die("_mzd_mul_naive: dimension mismatch.");
  if (gf2_require_device()) {
    std::fprintf(stderr, "m4ri_hip: _mzd_mul_naive failed: %s\n", gf2_last_error());
    return nullptr;
  }
  if (A->nrows == 0 || Bt->nrows == 0) return C;
  gf2_cache_forget(C);  // about to be overwritten
  {
    const long long lim = gf2_small_work_limit();
    if (lim > 0 && (long long)A->nrows * Bt->nrows * A->width <= lim && !gf2_cache_lookup(A) && !gf2_cache_lookup(Bt))
      return gf2_mul_nt_host_small(C, A, Bt, clear == 0) == 0 ? C : nullptr;  // size dispatch, see host_mul_on
  }
  PinnedDevice pin;  // M4RI_HIP_DEVICES = one ordinal: run there
  hipStream_t s;
  if (gf2_private_stream(&s)) return nullptr;
  int rc;
  {
    DMatOwner dA, dB, dC;
    rc = gf2_to_device(dA, A, s, true);
    if (!rc) rc = gf2_to_device(dB, Bt, s, true);
    if (!rc) rc = gf2_to_device(dC, C, s, clear == 0);
    if (!rc) rc = gf2_mul_nt_dev(&dC.d, &dA.d, &dB.d, clear == 0, s);
    if (!rc) rc = gf2_dmat_download(C, &dC.d, s);
    if (rc) (void)hipStreamSynchronize(s);
  }
  if (rc) {
    std::fprintf(stderr, "m4ri_hip: _mzd_mul_naive failed: %s\n", gf2_last_error());
    return nullptr;
  }
  return C;
}

extern "C" mzd_t *_mzd_mul_va(mzd_t *C, mzd_t const *v, mzd_t const *A, int clear) {
  if (!C) gf2_die("_mzd_mul_va: C must be preallocated.");
  return host_mul(C, v, A, clear == 0, GF2_ALGO_M4RM, 0, "_mzd_mul_va");
}

