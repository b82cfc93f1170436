// gf2_ple.hip -- PLE / PLUQ factorisation on the device, LAPACK-style row and column permutations, and the PLUQ solve
// (include/m4ri_hip.h: gf2_ple_dev, gf2_apply_p_dev, gf2_pluq_solve_left_dev).
//
// The factorisation is block-recursive over columns (M4RI's own structure).  PLE of rows [r0, m) and columns [c0, c1):
//   <= 64 columns: the panel (one word column): ple_panel_scan finds every chunk's row rank profile, ple_panel_pivots merges
//   the chunks in row order and runs the column-greedy elimination on the <= 64 pivot rows, ple_panel_apply writes every row's
//   L word (its coordinates in the basis E) and the panel's row order.
//   otherwise, split at a multiple of 64: left half; gather the right half's rows by the left order; E12 = L11^-1 A12
//   (gf2_trsm_dev, gf2_trsm.hip: block inverses and products); A22 ^= L21 E12 (gf2_mul_dev, the n^3 part); right half; gather L21's rows
//   by the right order; move the right L next to the left one (ple_compress_*).
// Non-pivot rows keep their relative order at every level, so the pivot rows are the row rank profile (the contract in
// INTEGRATION.md section 3).  Every kernel masks the excess bits of a row's last word: windows of dirty parents stay intact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "dev_args.h"
#include "gf2_kernels.h"

typedef uint64_t u64;

namespace {

constexpr int PANEL_CHUNK = 1024;  // rows per wave of ple_panel_scan

__device__ __forceinline__ u64 rdlane(u64 v, int lane) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}

// Reduces each lane's x against `basis` (lane b holds the vector with lowest set bit b, or 0) and inserts, in lane order, the
// lanes whose residue is non-zero.  Returns the ballot of inserted lanes; `nb` counts the basis vectors.
__device__ __forceinline__ u64 wave_insert(u64 &basis, u64 x, bool valid, int &nb) {
  const int lane = threadIdx.x & 63;
  for (int b = 0; b < 64; ++b) {
    const u64 v = rdlane(basis, b);
    if (v && ((x >> b) & 1)) x ^= v;
  }
  if (!valid) x = 0;
  u64 inserted = 0;
  u64 live = __ballot(x != 0);
  while (live) {
    const int f = __builtin_ctzll(live);
    const u64 xf = rdlane(x, f);
    const int lead = __builtin_ctzll(xf);
    if (lane == lead) basis = xf;
    inserted |= 1ull << f;
    ++nb;
    if (lane > f && ((x >> lead) & 1)) x ^= xf;
    live = __ballot(lane > f && x != 0);
  }
  return inserted;
}

// Phase 1: chunk c (PANEL_CHUNK rows from row c * PANEL_CHUNK of col[]) -> its row rank profile (<= 64 local indices).
__global__ void __launch_bounds__(64) ple_panel_scan(const u64 *col, int cnt, u64 vmask, int *cand) {
  const int lane = threadIdx.x;
  const int lo = blockIdx.x * PANEL_CHUNK, hi = min(cnt, lo + PANEL_CHUNK);
  const int full = __builtin_popcountll(vmask);
  u64 basis = 0;
  int nb = 0;
  int *out = cand + (size_t)blockIdx.x * 65;
  for (int base = lo; base < hi && nb < full; base += 64) {
    const int row = base + lane;
    const bool valid = row < hi;
    const u64 x = valid ? (col[row] & vmask) : 0;
    const int before = nb;
    u64 ins = wave_insert(basis, x, valid, nb);
    if ((ins >> lane) & 1) out[1 + before + __builtin_popcountll(ins & ((1ull << lane) - 1))] = row;
  }
  if (lane == 0) out[0] = nb;
}

// Phase 2 (one wave): merge the chunk candidates in row order -> the panel's row rank profile S; column-greedy elimination of S
// -> tab: [0, 64) E words, [64, 128) pivot column of E_k (as u64), [128, 192) local row of E_k, [192, 256) S sorted, [256] rank.
// Q of the panel goes to qcol[k] = colbase + column, the rank to rank_out.
__global__ void __launch_bounds__(64) ple_panel_pivots(const u64 *col, int nchunk, u64 vmask, const int *cand, u64 *tab,
                                                       int *qcol, int colbase) {
  const int lane = threadIdx.x;
  const int full = __builtin_popcountll(vmask);
  u64 basis = 0;
  int nb = 0;
  int srow = -1;  // lane k: k-th row of S
  for (int c = 0; c < nchunk && nb < full; ++c) {
    const int *cc = cand + (size_t)c * 65;
    const int n = cc[0];
    const int row = lane < n ? cc[1 + lane] : 0;
    const u64 x = lane < n ? (col[row] & vmask) : 0;
    const int before = nb;
    const u64 ins = wave_insert(basis, x, lane < n, nb);
    // lane before + j of S receives the j-th inserted lane's row
    for (u64 t = ins; t; t &= t - 1) {
      const int f = __builtin_ctzll(t);
      const int r = __builtin_amdgcn_readlane(row, f);
      if (lane == before + __builtin_popcountll(ins & ((1ull << f) - 1))) srow = r;
    }
  }
  const int rank = nb;
  // column greedy on S in row order: pivot of column c = first remaining S row with bit c
  u64 y = lane < rank ? (col[srow] & vmask) : 0;
  bool remaining = lane < rank;
  int k = 0;
  for (int c = 0; c < 64 && k < rank; ++c) {
    const u64 has = __ballot(remaining && ((y >> c) & 1));
    if (!has) continue;
    const int p = __builtin_ctzll(has);
    const u64 e = rdlane(y, p);
    const int prow = __builtin_amdgcn_readlane(srow, p);
    if (lane == p) remaining = false;
    if (remaining && ((y >> c) & 1)) y ^= e;
    if (lane == 0) {
      tab[k] = e;
      tab[64 + k] = (u64)c;
      tab[128 + k] = (u64)prow;
      qcol[k] = colbase + c;
    }
    ++k;
  }
  tab[192 + lane] = lane < rank ? (u64)srow : ~0ull;
  if (lane == 0) tab[256] = (u64)rank;
}

// Phase 3: position i of the panel's rows takes source row pi(i) (pivots by pivot column, then the other rows in order);
// its word becomes L bits (+ E_i for a pivot).  Reads the copy col[], writes A's word column (excess bits kept) and pi.
__global__ void __launch_bounds__(256) ple_panel_apply(const u64 *col, int cnt, u64 vmask, const u64 *tab, u64 *A, long long lda,
                                                       int *pi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const int rank = (int)tab[256];
  int src;
  if (i < rank) {
    src = (int)tab[128 + i];
  } else {
    src = i - rank;
    for (int j = 0; j < rank; ++j)
      if ((int)tab[192 + j] <= src) ++src;
  }
  u64 x = col[src] & vmask, c = 0;
  for (int k = 0; k < rank; ++k) {
    if ((x >> tab[64 + k]) & 1) {
      x ^= tab[k];
      c |= 1ull << k;
    }
  }
  u64 out = i < rank ? ((c & ((1ull << i) - 1)) | tab[i]) : c;
  u64 *dst = A + (long long)i * lda;
  *dst = (*dst & ~vmask) | (out & vmask);
  pi[i] = src;
}

// dst[i][w] = src[perm ? perm[i] : i][w] (src null: 0) for w < words; the last word only under lastmask
__global__ void __launch_bounds__(256) ple_gather(u64 *dst, long long ldd, const u64 *src, long long lds_, const int *perm, int rows,
                                                  int words, u64 lastmask) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)rows * words) return;
  const int i = (int)(t / words), w = (int)(t % words);
  const u64 m = w == words - 1 ? lastmask : ~0ull;
  const u64 v = src ? src[(long long)(perm ? perm[i] : i) * lds_ + w] : 0;
  u64 *d = dst + (long long)i * ldd + w;
  *d = (*d & ~m) | (v & m);
}

// pi[j] = stash[r1 + pi[j]] (composition of the left and the right row order of a node, local to the node)
__global__ void __launch_bounds__(256) ple_compose(int *pi, const int *stash, int r1, int cnt) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < cnt) pi[j] = stash[r1 + pi[j]];
}

// L of the right half (bit columns [sbit, sbit + w_i) of row i, w_i = min(i, r2)) -> scratch S (dense, sw words per row)
__global__ void __launch_bounds__(256) ple_compress_extract(const u64 *A, long long lda, int rows, int sbit, int r2, u64 *S, int sw) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)rows * sw) return;
  const int i = (int)(t / sw), q = (int)(t % sw);
  const int wi = min(i, r2);
  const int b0 = q * 64;
  u64 v = 0;
  if (b0 < wi) {
    const u64 *row = A + (long long)i * lda;
    const int bit = sbit + b0, w = bit >> 6, sh = bit & 63;
    const int n = wi - b0;
    v = row[w] >> sh;
    if (sh && sh + n > 64) v |= row[w + 1] << (64 - sh);  // only when wanted bits lie in it: word w may be the row's last
    if (n < 64) v &= (1ull << n) - 1;
  }
  S[(long long)i * sw + q] = v;
}

// row i: clear bits [sbit, sbit + w_i), then OR in the scratch bits at [dbit, dbit + w_i); one thread per word of [wlo, whi)
__global__ void __launch_bounds__(256) ple_compress_place(u64 *A, long long lda, int rows, int sbit, int dbit, int r2, const u64 *S,
                                                          int sw, int wlo, int nwords) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)rows * nwords) return;
  const int i = (int)(t / nwords), w = wlo + (int)(t % nwords);
  const int wi = min(i, r2);
  if (wi == 0) return;
  auto range = [&](int lo, int n) -> u64 {  // bits [lo, lo + n) that fall into word w
    const long long a = std::max<long long>(lo, (long long)w * 64), b = std::min<long long>((long long)lo + n, (long long)w * 64 + 64);
    if (a >= b) return 0;
    const int s = (int)(a - (long long)w * 64), len = (int)(b - a);
    return (len == 64 ? ~0ull : ((1ull << len) - 1)) << s;
  };
  const u64 clr = range(sbit, wi), put = range(dbit, wi);
  if (!clr && !put) return;
  u64 v = 0;
  if (put) {  // destination bit p of word w comes from scratch bit (w * 64 + p - dbit)
    const long long o = (long long)w * 64 - dbit;  // scratch bit of this word's bit 0 (may be negative)
    const u64 *s = S + (long long)i * sw;
    if (o >= 0) {
      const int q = (int)(o >> 6), sh = (int)(o & 63);
      v = s[q] >> sh;
      if (sh && q + 1 < sw) v |= s[q + 1] << (64 - sh);
    } else {
      v = s[0] << (int)(-o);
    }
    v &= put;
  }
  u64 *d = A + (long long)i * lda + w;
  *d = (*d & ~clr) | v;
}

// ple_tri: mode 0: dst[j] = src[j] without the bits below j (and only bits < ncols); mode 1: dst[j] keeps its bits below j
// (and beyond ncols), takes src[j]'s from bit j on.  rows x words, one thread per word.
__global__ void __launch_bounds__(256) ple_tri(u64 *dst, long long ldd, const u64 *src, long long lds_, int rows, int words,
                                               u64 lastmask, int mode) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)rows * words) return;
  const int j = (int)(t / words), w = (int)(t % words);
  const u64 valid = w == words - 1 ? lastmask : ~0ull;
  const int lo = j - w * 64;  // bits of this word below column j
  const u64 low = lo <= 0 ? 0 : (lo >= 64 ? ~0ull : ((1ull << lo) - 1));
  const u64 v = src[(long long)j * lds_ + w];
  u64 *d = dst + (long long)j * ldd + w;
  if (mode == 0) *d = v & ~low & valid;
  else *d = (*d & (low | ~valid)) | (v & ~low & valid);
}

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------

inline int words_of(long long bits) { return (int)((bits + 63) >> 6); }
inline u64 last_mask(long long bits) { return (bits & 63) ? ((1ull << (bits & 63)) - 1) : ~0ull; }
inline long long even_ld(long long w) { return (w + 1) & ~1ll; }  // device matrices keep even row strides
inline unsigned grid_of(long long n, int b) { return (unsigned)((n + b - 1) / b); }


// Scratch of this file comes from the block cache (DevBuf), whose free is not stream-ordered: a scope that holds such a block ends
// behind a wait for its stream on every path, the error returns included.  Declared after the buffers, so destroyed before them.
struct DrainOnExit {
  hipStream_t s;
  ~DrainOnExit() {
    if (hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
  }
};

inline gf2_dmat win(const gf2_dmat &A, long long r, long long c, int rows, int cols) {
  // c: multiple of 64
  return gf2_dmat{static_cast<u64 *>(A.data) + r * A.ld + (c >> 6), A.ld, rows, cols};
}

// dst rows [0, rows) x words = src rows perm[i] (perm null: identity) through scratch when they alias; lastmask on the last word
int gather_rows(const gf2_dmat &D, const int *perm_dev, int rows, int words, u64 lastmask, u64 *scratch, hipStream_t s) {
  if (rows <= 0 || words <= 0) return 0;
  HIP_TRY(hipMemcpy2DAsync(scratch, (size_t)words * 8, D.data, (size_t)D.ld * 8, (size_t)words * 8, rows, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(ple_gather, dim3(grid_of((long long)rows * words, 256)), dim3(256), 0, s, static_cast<u64 *>(D.data), D.ld,
                     scratch, (long long)words, perm_dev, rows, words, lastmask);
  HIP_TRY(hipGetLastError());
  return 0;
}

struct PleCtx {
  gf2_dmat A;
  int m, n;
  hipStream_t s;
  int *pi;                    // device, m: row order of the current node, local to its first row
  int *qcol;                  // device, min(m, n): pivot columns
  std::vector<int *> stash;   // device, m each: one per recursion depth (a node keeps its left half's order there)
  u64 *scratch;               // device: m * ceil(words / 2) + m words (gathers, the panel column, compress scratch)
  int *cand;                  // device: ceil(m / PANEL_CHUNK) * 65
  u64 *tab;                   // device: 257 words
  u64 *rank_host;             // pinned
};

int panel(PleCtx &c, int r0, int c0, int c1, int *rank) {
  const int cnt = c.m - r0;
  *rank = 0;
  if (cnt <= 0) return 0;
  const u64 vmask = last_mask(c1 - c0);
  u64 *A0 = static_cast<u64 *>(c.A.data) + (long long)r0 * c.A.ld + (c0 >> 6);
  u64 *col = c.scratch;
  HIP_TRY(hipMemcpy2DAsync(col, 8, A0, (size_t)c.A.ld * 8, 8, cnt, hipMemcpyDeviceToDevice, c.s));
  const int nchunk = (cnt + PANEL_CHUNK - 1) / PANEL_CHUNK;
  hipLaunchKernelGGL(ple_panel_scan, dim3(nchunk), dim3(64), 0, c.s, col, cnt, vmask, c.cand);
  hipLaunchKernelGGL(ple_panel_pivots, dim3(1), dim3(64), 0, c.s, col, nchunk, vmask, c.cand, c.tab, c.qcol + r0, c0);
  hipLaunchKernelGGL(ple_panel_apply, dim3(grid_of(cnt, 256)), dim3(256), 0, c.s, col, cnt, vmask, c.tab, A0, c.A.ld, c.pi + r0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c.rank_host, c.tab + 256, 8, hipMemcpyDeviceToHost, c.s));
  HIP_TRY(hipStreamSynchronize(c.s));
  *rank = (int)*c.rank_host;
  return 0;
}

int ple_rec(PleCtx &c, int r0, int c0, int c1, int depth, int *rank) {
  *rank = 0;
  if (r0 >= c.m || c1 <= c0) return 0;
  if (c1 - c0 <= 64) return panel(c, r0, c0, c1, rank);
  const int cmid = c0 + 64 * ((words_of(c1 - c0) + 1) / 2);
  const int cnt = c.m - r0;
  int r1 = 0, r2 = 0;
  GF2_RC(ple_rec(c, r0, c0, cmid, depth + 1, &r1));
  int *st = c.stash[depth];
  HIP_TRY(hipMemcpyAsync(st + r0, c.pi + r0, (size_t)cnt * sizeof(int), hipMemcpyDeviceToDevice, c.s));
  // right half in the left half's row order
  gf2_dmat R = win(c.A, r0, cmid, cnt, c1 - cmid);
  GF2_RC(gather_rows(R, st + r0, cnt, words_of(c1 - cmid), last_mask(c1 - cmid), c.scratch, c.s));
  if (r1 > 0) {
    gf2_dmat L11 = win(c.A, r0, c0, r1, r1), A12 = win(c.A, r0, cmid, r1, c1 - cmid);
    GF2_RC(gf2_trsm_dev(&L11, &A12, 0, 0, c.s));  // E12 = L11^-1 A12
    if (cnt > r1) {
      gf2_dmat C = win(c.A, r0 + r1, cmid, cnt - r1, c1 - cmid), L = win(c.A, r0 + r1, c0, cnt - r1, r1),
               E = win(c.A, r0, cmid, r1, c1 - cmid);
      GF2_RC(gf2_mul_dev(&C, &L, &E, 1, 0, 0, c.s));  // A22 ^= L21 E12
    }
  }
  if (cnt > r1) {
    GF2_RC(ple_rec(c, r0 + r1, cmid, c1, depth + 1, &r2));
    const int rest = cnt - r1;
    // left half's rows below the left pivots in the right half's order (whole words: [c0, cmid) lies inside the matrix)
    gf2_dmat Lh = win(c.A, r0 + r1, c0, rest, cmid - c0);
    GF2_RC(gather_rows(Lh, c.pi + r0 + r1, rest, words_of(cmid - c0), ~0ull, c.scratch, c.s));
    hipLaunchKernelGGL(ple_compose, dim3(grid_of(rest, 256)), dim3(256), 0, c.s, c.pi + r0 + r1, st + r0, r1, rest);
    HIP_TRY(hipGetLastError());
    if (r2 > 0 && r1 < cmid - c0) {  // right L from column cmid to column c0 + r1
      const int sw = words_of(r2);
      u64 *row0 = static_cast<u64 *>(c.A.data) + (long long)(r0 + r1) * c.A.ld;
      hipLaunchKernelGGL(ple_compress_extract, dim3(grid_of((long long)rest * sw, 256)), dim3(256), 0, c.s, row0, c.A.ld, rest,
                         cmid, r2, c.scratch, sw);
      const int wlo = (c0 + r1) >> 6, whi = words_of(cmid + r2);
      hipLaunchKernelGGL(ple_compress_place, dim3(grid_of((long long)rest * (whi - wlo), 256)), dim3(256), 0, c.s, row0, c.A.ld,
                         rest, cmid, c0 + r1, r2, c.scratch, sw, wlo, whi - wlo);
      HIP_TRY(hipGetLastError());
    }
  }
  *rank = r1 + r2;
  return 0;
}

// transposition list -> gather map: position i of the result takes row map[i] of the input
std::vector<int> perm_map(const int *P, int len, int rows, bool descending) {
  std::vector<int> at(rows);
  for (int i = 0; i < rows; ++i) at[i] = i;
  const int n = std::min(len, rows);
  for (int t = 0; t < n; ++t) {
    const int i = descending ? n - 1 - t : t;
    const int j = P[i];  // in [0, rows): every caller validates the list first
    if (j != i) std::swap(at[i], at[j]);
  }
  return at;
}

int apply_rows(const gf2_dmat &A, const std::vector<int> &map, hipStream_t s) {
  const int rows = A.nrows, words = words_of(A.ncols);
  if (rows == 0 || words == 0) return 0;
  DevBuf dm, sc;
  DrainOnExit drain{s};
  GF2_RC(dm.alloc((size_t)rows * sizeof(int)));
  GF2_RC(sc.alloc((size_t)rows * words * 8));
  HIP_TRY(hipMemcpyAsync(dm.p, map.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice, s));
  GF2_RC(gather_rows(A, dm.as<int>(), rows, words, last_mask(A.ncols), sc.as<u64>(), s));
  HIP_TRY(hipStreamSynchronize(s));  // map and scratch are freed on return
  return 0;
}

}  // namespace

// column permutation: A^T, its rows gathered, transposed back, copied into A under the masks (synchronous)
static int apply_cols_dev(const gf2_dmat &A, const std::vector<int> &map, hipStream_t s) {
  const int m = A.nrows, n = A.ncols;
  if (m == 0 || n == 0) return 0;
  const long long tw = even_ld(words_of(m)), aw = even_ld(words_of(n));
  DevBuf t1, t2, dm;
  DrainOnExit drain{s};
  GF2_RC(t1.alloc((size_t)std::max<long long>((long long)n * tw, (long long)m * aw) * 8));
  GF2_RC(t2.alloc((size_t)n * tw * 8));
  GF2_RC(dm.alloc((size_t)n * sizeof(int)));
  HIP_TRY(hipMemcpyAsync(dm.p, map.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
  gf2_dmat Ac = A, T{t1.as<u64>(), tw, n, m};
  GF2_RC(gf2_transpose_dev(&T, &Ac, s));  // T = A^T
  hipLaunchKernelGGL(ple_gather, dim3(grid_of((long long)n * tw, 256)), dim3(256), 0, s, t2.as<u64>(), tw, t1.as<u64>(), tw,
                     dm.as<int>(), n, (int)tw, ~0ull);
  HIP_TRY(hipGetLastError());
  gf2_dmat G{t2.as<u64>(), tw, n, m}, U{t1.as<u64>(), aw, m, n};
  GF2_RC(gf2_transpose_dev(&U, &G, s));  // U = (gathered A^T)^T
  hipLaunchKernelGGL(ple_gather, dim3(grid_of((long long)m * words_of(n), 256)), dim3(256), 0, s, static_cast<u64 *>(A.data), A.ld,
                     t1.as<u64>(), aw, (const int *)nullptr, m, words_of(n), last_mask(n));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

extern "C" int gf2_apply_p_dev(gf2_dmat *A, const int *P, int len, int right, int trans, void *stream) {
  static const char fn[] = "gf2_apply_p_dev";
  if (int rc = gf2_check_mat(fn, "A", A)) return rc;
  if (len < 0) return gf2_bad_arg(fn, "len is negative");
  if (len > 0) GF2_RC(gf2_refuse_null(fn, "P", P));
  for (int i = 0, n = std::min(len, right ? A->ncols : A->nrows); i < n; ++i)
    if (P[i] < 0 || P[i] >= (right ? A->ncols : A->nrows)) return gf2_bad_arg(fn, "P[i] out of range");
  if (A->nrows == 0 || A->ncols == 0) return 0;
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!right) {  // left: ascending swaps; left_trans: descending
    return apply_rows(*A, perm_map(P, len, A->nrows, trans != 0), s);
  }
  // right: column swaps descending; right_trans: ascending.  Column c of the result = column map[c] of the input.
  return apply_cols_dev(*A, perm_map(P, len, A->ncols, trans == 0), s);
}

// pivot order sigma (sigma[i] = input row at position i) -> transposition list for mzd_apply_p_left
static void sigma_to_transpositions(const std::vector<int> &sigma, int *P) {
  const int m = (int)sigma.size();
  std::vector<int> pos(m), at(m);
  for (int i = 0; i < m; ++i) pos[i] = at[i] = i;
  for (int i = 0; i < m; ++i) {
    const int p = pos[sigma[i]];
    P[i] = p;
    const int a = at[i], b = at[p];
    std::swap(at[i], at[p]);
    pos[a] = p;
    pos[b] = i;
  }
}

extern "C" int gf2_ple_dev(gf2_dmat *A, int pluq, int *P, int *Q, int *rank, void *stream) {
  static const char fn[] = "gf2_ple_dev";
  if (int rc = gf2_check_mat(fn, "A", A)) return rc;
  GF2_RC(gf2_refuse_null(fn, "rank", rank));
  if ((A->nrows && !P) || (A->ncols && !Q)) return gf2_bad_arg(fn, "P or Q is null");
  const int m = A->nrows, n = A->ncols;
  *rank = 0;
  for (int i = 0; i < m; ++i) P[i] = i;
  for (int j = 0; j < n; ++j) Q[j] = j;
  if (m == 0 || n == 0) return 0;
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int aw = words_of(n);
  DevBuf pi, qc, sc, cand, tab, stash, eb;
  DrainOnExit drain{s};
  GF2_RC(pi.alloc((size_t)m * sizeof(int)));
  GF2_RC(qc.alloc((size_t)std::min(m, n) * sizeof(int)));
  const long long swords = std::max<long long>((long long)m * ((aw + 1) / 2), (long long)m * (words_of(std::min(m, n)) + 1));
  GF2_RC(sc.alloc((size_t)swords * 8));
  GF2_RC(cand.alloc((size_t)((m + PANEL_CHUNK - 1) / PANEL_CHUNK) * 65 * sizeof(int)));
  GF2_RC(tab.alloc(257 * 8));
  u64 *rank_host = nullptr;
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&rank_host), 8, 0));
  int depth = 1;
  for (int w = aw; w > 1; w = (w + 1) / 2) ++depth;  // levels of the column recursion
  GF2_RC(stash.alloc((size_t)depth * m * sizeof(int)));
  PleCtx c{*A, m, n, s, pi.as<int>(), qc.as<int>(), {}, sc.as<u64>(), cand.as<int>(), tab.as<u64>(), rank_host};
  for (int d = 0; d < depth; ++d) c.stash.push_back(stash.as<int>() + (size_t)d * m);
  int r = 0;
  int rc = ple_rec(c, 0, 0, n, 0, &r);
  std::vector<int> sigma(m), q(std::max(r, 1));
  if (!rc) {
    hipError_t e = hipMemcpyAsync(sigma.data(), c.pi, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && r > 0) e = hipMemcpyAsync(q.data(), c.qcol, (size_t)r * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = gf2_fail_hip(e, "gf2_ple_dev: download of the permutations");
  } else {
    (void)hipStreamSynchronize(s);
  }
  (void)hipHostFree(rank_host);
  if (rc) return rc;
  sigma_to_transpositions(sigma, P);
  for (int k = 0; k < r; ++k) Q[k] = q[k];
  *rank = r;
  if (pluq && r > 0) {
    // U = E with the transpositions of Q applied to its columns in ascending order (mzd_apply_p_right_trans); the bits of E below
    // the diagonal are zero, so the swaps that would touch L are no-ops and the whole rows can be permuted
    const long long eld = even_ld(aw);
    GF2_RC(eb.alloc((size_t)r * eld * 8));
    gf2_dmat E{eb.as<u64>(), eld, r, n};
    hipLaunchKernelGGL(ple_tri, dim3(grid_of((long long)r * aw, 256)), dim3(256), 0, s, eb.as<u64>(), eld,
                       static_cast<const u64 *>(A->data), A->ld, r, aw, last_mask(n), 0);
    HIP_TRY(hipGetLastError());
    GF2_RC(apply_cols_dev(E, perm_map(Q, n, n, false), s));
    hipLaunchKernelGGL(ple_tri, dim3(grid_of((long long)r * aw, 256)), dim3(256), 0, s, static_cast<u64 *>(A->data), A->ld,
                       eb.as<const u64>(), eld, r, aw, last_mask(n), 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

extern "C" int gf2_pluq_solve_left_dev(gf2_dmat const *A, int rank, const int *P, const int *Q, gf2_dmat *B, int check,
                                       int *inconsistent, void *stream) {
  static const char fn[] = "gf2_pluq_solve_left_dev";
  if (gf2_check_mat(fn, "A", A) || gf2_check_mat(fn, "B", B)) return -1;
  GF2_RC(gf2_refuse_null(fn, "inconsistent", inconsistent));
  if ((A->nrows && !P) || (A->ncols && !Q)) return gf2_bad_arg(fn, "P or Q is null");
  const int m = A->nrows, n = A->ncols, kb = B->ncols;
  *inconsistent = 0;
  if (B->nrows < m || B->nrows < n) return gf2_fail_msg("gf2_pluq_solve_left_dev: B needs max(A nrows, A ncols) rows");
  if (rank < 0 || rank > std::min(m, n)) return gf2_fail_msg("gf2_pluq_solve_left_dev: rank out of range");
  if (m == 0 || n == 0 || kb == 0) return 0;
  for (int i = 0; i < m; ++i)
    if (P[i] < 0 || P[i] >= m) return gf2_fail_msg("gf2_pluq_solve_left_dev: P[i] out of range");
  for (int j = 0; j < n; ++j)
    if (Q[j] < 0 || Q[j] >= n) return gf2_fail_msg("gf2_pluq_solve_left_dev: Q[j] out of range");
  if (int rc = gf2_refuse_overlap(fn, "B", B, "A", A)) return rc;  // B is rewritten step by step while A is still read
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int bw = words_of(kb);
  const u64 bmask = last_mask(kb);
  gf2_dmat Bm = win(*B, 0, 0, m, kb);
  GF2_RC(apply_rows(Bm, perm_map(P, m, m, false), s));                  // P B
  gf2_dmat T11 = win(*A, 0, 0, rank, rank), Y = win(*B, 0, 0, rank, kb);  // L11 and U11 share the block: gf2_trsm_dev reads one strict triangle
  GF2_RC(gf2_trsm_dev(&T11, &Y, 0, 0, s));                               // Y = L11^-1 (P B)[0, r)
  if (check && rank < m) {
    gf2_dmat C = win(*B, rank, 0, m - rank, kb), L = win(*A, rank, 0, m - rank, rank);
    if (rank > 0) GF2_RC(gf2_mul_dev(&C, &L, &Y, 1, 0, 0, s));          // rows r.. of P B minus L21 Y: zero iff consistent
    DevBuf flag;
    DrainOnExit drain{s};
    GF2_RC(flag.alloc(sizeof(int)));
    int h = 0;
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    HIP_TRY(gf2k_any_nonzero(static_cast<const u64 *>(B->data), B->ld, rank, m, kb, flag.as<int>(), s));
    HIP_TRY(hipMemcpyAsync(&h, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *inconsistent = h != 0;
  }
  GF2_RC(gf2_trsm_dev(&T11, &Y, 1, 0, s));                               // Z = U11^-1 Y, free variables 0
  if (B->nrows > rank) {
    hipLaunchKernelGGL(ple_gather, dim3(grid_of((long long)(B->nrows - rank) * bw, 256)), dim3(256), 0, s,
                       static_cast<u64 *>(B->data) + (long long)rank * B->ld, B->ld, (const u64 *)nullptr, 0ll, (const int *)nullptr,
                       B->nrows - rank, bw, bmask);
    HIP_TRY(hipGetLastError());
  }
  gf2_dmat Bn = win(*B, 0, 0, n, kb);
  return apply_rows(Bn, perm_map(Q, n, n, true), s);                     // X = Q^T Z (synchronous)
}
