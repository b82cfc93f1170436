// gf2_nullspace.hip -- null space basis of a device matrix (include/m4ri_hip.h: gf2_nullspace_dev; contract: INTEGRATION.md section 3;
// DESIGN.md section 7.4).
//
// A (m x n, rank r) is brought to its reduced row echelon form E by the elimination of gf2_elim.hip, whose pivot columns p_0 < ... <
// p_{r-1} stay on the device.  With the free columns f_0 < ... < f_{n-r-1}, the basis K (n x (n - r)) is
//   row f_j = the unit vector e_j,      row p_i = the bits of row i of E at the free columns, in order.
// Two launches follow the elimination:
//   1. nullspace_prepare, one thread per 64-column source word q.  The pivot columns are sorted, so a binary search gives the number of
//      pivots left of the word -- and with it the number of free columns left of it -- without a scan.  The thread writes the word's
//      free-column mask (a packed array: neighbouring lanes of the next launch read neighbouring masks) and the six control masks of a
//      parallel-suffix bit compress under that mask (the column mask is the same for every row: they are computed once, not per row), the row kind of K's 64 rows c = 64 q + b (pivot row index i, or ~j for free
//      index j), and, if free index 64 w falls into the word, the start entry of output word w: (q, free bits of q before it).
//   2. nullspace_assemble, one thread per output word (row c, word w): a workgroup is a 2-D tile of rows x words (threadIdx.x walks the
//      words, so the stores are coalesced along a row of K, and no thread divides to find its row).  A pivot row
//      walks the words of E's row i from the start entry of w, compresses each under its mask and funnels the result into the output
//      word until it is full; a word whose mask is all ones needs no compress (a random matrix has its pivots first: every source word
//      but one is of that kind, and neighbouring threads read neighbouring words).  A free row writes its unit word or zero.
// Every word of K is written, the excess bits of its last word as zeros (a compress leaves zeros above the bits it gathered).
#include <hip/hip_runtime.h>

#include "dev_args.h"
#include "gf2_kernels.h"

typedef uint64_t u64;

namespace {

constexpr int CTL_WORDS = 6;  // per source word: the six moves of the compress under its free-column mask

__device__ __forceinline__ u64 low_bits(int n) { return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1)); }

// x's bits under m, moved together at the low end (mv: the six moves that belong to m)
__device__ __forceinline__ u64 compress(u64 x, u64 m, const u64 *__restrict__ mv) {
  x &= m;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const u64 t = x & mv[i];
    x = (x ^ t) | (t >> (1 << i));
  }
  return x;
}

// n columns in nw words, r sorted pivot columns; K has kw words per row.  fmask: nw words, ctl: nw * CTL_WORDS words, rowinfo: n ints,
// start: kw int2.
__global__ void __launch_bounds__(256) nullspace_prepare(const int *__restrict__ pivcols, int r, int n, int nw, int kw,
                                                         u64 *__restrict__ fmask, u64 *__restrict__ ctl, int *__restrict__ rowinfo, int2 *__restrict__ start) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nw) return;
  const long long c0 = (long long)q * 64;
  int lo = 0, hi = r;  // first pivot at or right of column c0
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (pivcols[mid] < c0) lo = mid + 1;
    else hi = mid;
  }
  const int piv_before = lo;
  u64 pm = 0;
  for (int k = lo; k < r && pivcols[k] < c0 + 64; ++k) pm |= 1ull << (pivcols[k] - c0);
  const int cols = n - c0 < 64 ? (int)(n - c0) : 64;
  const u64 fm = ~pm & low_bits(cols);
  const int free_before = (int)(c0 - piv_before);
  u64 *e = ctl + (long long)q * CTL_WORDS;
  fmask[q] = fm;
  {  // Hacker's Delight 7-4: the moves depend on the mask alone
    u64 m = fm, mk = ~fm << 1;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      u64 mp = mk ^ (mk << 1);
      mp ^= mp << 2;
      mp ^= mp << 4;
      mp ^= mp << 8;
      mp ^= mp << 16;
      mp ^= mp << 32;
      const u64 mv = mp & m;
      m = (m ^ mv) | (mv >> (1 << i));
      mk &= ~mp;
      e[i] = mv;
    }
  }
  int i = piv_before, j = free_before;
  for (int b = 0; b < cols; ++b) rowinfo[c0 + b] = ((fm >> b) & 1) ? ~(j++) : i++;
  // free indices [free_before, free_before + popcount) live here: at most one multiple of 64 among them
  const int w = (free_before + 63) >> 6;
  if (w < kw && w * 64 < free_before + __popcll(fm)) start[w] = make_int2(q, w * 64 - free_before);
}

// K[c][w] for c < n, w < kw; d = n - r columns of K.  E: the reduced echelon form, lde words between rows.  blockDim.x * blockDim.y = 256:
// blockDim.x words (a power of two) of blockDim.y rows; rows along grid.x (grid.y ends at 65535), words along grid.y.
__global__ void __launch_bounds__(256) nullspace_assemble(const u64 *__restrict__ E, long long lde, int nw, const u64 *__restrict__ fmask,
                                                          const u64 *__restrict__ ctl,
                                                          const int *__restrict__ rowinfo, const int2 *__restrict__ start,
                                                          u64 *__restrict__ K, long long ldk, int n, int kw, int d) {
  const long long c = (long long)blockIdx.x * blockDim.y + threadIdx.y;
  const int w = blockIdx.y * blockDim.x + threadIdx.x;
  if (c >= n || w >= kw) return;
  const int info = rowinfo[c];
  u64 out = 0;
  if (info < 0) {
    const int j = ~info;
    if ((j >> 6) == w) out = 1ull << (j & 63);
  } else {
    const u64 *row = E + (long long)info * lde;
    const int need = d - w * 64 < 64 ? d - w * 64 : 64;  // bits of this output word
    const int2 st = start[w];
    int q = st.x, skip = st.y, have = 0;
    while (have < need && q < nw) {
      const u64 fm = fmask[q];
      if (fm) {
        u64 x = row[q];
        if (fm != ~0ull) x = compress(x, fm, ctl + (long long)q * CTL_WORDS);
        out |= (x >> skip) << have;  // skip < popcount(fm) <= 64 and have < 64
        have += __popcll(fm) - skip;
        skip = 0;
      }
      ++q;
    }
  }
  __builtin_nontemporal_store(out, K + c * ldk + w);  // written once, not read again here
}

inline int words_of(long long bits) { return (int)((bits + 63) >> 6); }

// gf2_prof_enable is on: events around the assembly launch; the last call's time on this thread
thread_local double tls_assemble_ms = 0;
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace

extern "C" int gf2_nullspace_dev(gf2_dmat *A, gf2_dmat *K, int *rank, int *pivot_cols, void *stream) {
  static const char fn[] = "gf2_nullspace_dev";
  if (int rc = gf2_check_mat(fn, "A", A)) return rc;
  GF2_RC(gf2_refuse_null(fn, "K", K));
  GF2_RC(gf2_refuse_null(fn, "rank", rank));
  const int n = A->ncols, nw = words_of(n);
  if (n > 0) GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  *rank = 0;
  *K = gf2_dmat{nullptr, 0, n, 0};
  if (n == 0) return 0;
  DevBuf piv;  // the elimination's own buffer of pivot columns, handed over
  if (int rc = gf2_rref_keep_pivots_dev(A, rank, pivot_cols, &piv.p, &piv.bytes, s)) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  const int *pivcols = static_cast<const int *>(piv.p);
  const int r = *rank, d = n - r;
  if (d == 0) return 0;
  const int kw = words_of(d);
  // one block: the masks, the control words, the start entries, the row kinds
  const size_t mask_bytes = (size_t)nw * sizeof(u64), ctl_bytes = (size_t)nw * CTL_WORDS * sizeof(u64), start_bytes = (size_t)kw * sizeof(int2);
  DevBuf prep;
  if (int rc = prep.alloc(mask_bytes + ctl_bytes + start_bytes + (size_t)n * sizeof(int))) return rc;
  u64 *fmask = static_cast<u64 *>(prep.p), *ctl = fmask + nw;
  int2 *start = reinterpret_cast<int2 *>(static_cast<char *>(prep.p) + mask_bytes + ctl_bytes);
  int *rowinfo = reinterpret_cast<int *>(static_cast<char *>(prep.p) + mask_bytes + ctl_bytes + start_bytes);
  if (int rc = gf2_dmat_alloc(K, n, d)) {
    *K = gf2_dmat{nullptr, 0, n, 0};
    return rc;
  }
  int wx = 1;  // words of a workgroup's tile: the power of two that covers a row of K, 256 at the most
  while (wx < kw && wx < 256) wx <<= 1;
  const int ry = 256 / wx;
  const dim3 grid((unsigned)((n + ry - 1) / ry), (unsigned)((kw + wx - 1) / wx));
  auto enqueue = [&]() -> int {
    if (grid.y > 65535u) return gf2_fail_msg("gf2_nullspace_dev: the basis is too wide for one launch");
    hipLaunchKernelGGL(nullspace_prepare, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, pivcols, r, n, nw, kw, fmask, ctl, rowinfo,
                       start);
    HIP_TRY(hipGetLastError());
    const bool prof = gf2_prof_is_on();
    EventPair ev;
    if (prof) {
      HIP_TRY(hipEventCreate(&ev.a));
      HIP_TRY(hipEventCreate(&ev.b));
      HIP_TRY(hipEventRecord(ev.a, s));
    }
    hipLaunchKernelGGL(nullspace_assemble, grid, dim3(wx, ry), 0, s, static_cast<const u64 *>(A->data), (long long)A->ld, nw, fmask, ctl,
                       rowinfo, start, static_cast<u64 *>(K->data), (long long)K->ld, n, kw, d);
    HIP_TRY(hipGetLastError());
    if (prof) HIP_TRY(hipEventRecord(ev.b, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (prof) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
      tls_assemble_ms = ms;
    }
    return 0;
  };
  if (int rc = enqueue()) {
    (void)hipStreamSynchronize(s);
    gf2_dmat_free(K);
    *K = gf2_dmat{nullptr, 0, n, 0};
    return rc;
  }
  return 0;
}

extern "C" double gf2_nullspace_last_assembly_ms(void) { return tls_assemble_ms; }
