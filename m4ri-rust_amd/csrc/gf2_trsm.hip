// gf2_trsm.hip -- triangular solves with a unit triangular matrix on the device (include/m4ri_hip.h: gf2_trsm_dev; contract:
// INTEGRATION.md section 3).
//
// No substitution chain runs against the right-hand side: every step of the solve is a product.
//   1. trsm_invert_blocks (one launch, one workgroup per block) inverts the d x d diagonal blocks of T into dense scratch.  A
//      wave inverts a 64 x 64 diagonal sub-block by 63 cross-lane substitution steps on the identity (lane i holds row i), then
//      the workgroup doubles: [[A, 0], [C, D]]^-1 = [[A^-1, 0], [D^-1 C A^-1, D^-1]] (upper: mirrored), the two 64-row x 64-bit
//      word products per wave as selected XORs of LDS rows (every lane reads the same word: a broadcast).  The kernel reads only
//      the strict triangle it is asked for: the diagonal counts as 1, the other triangle is masked away as the words are staged.
//   2. block recursion on the host: a leaf is (stored inverse) x (block of B) into scratch of the per-stream arena and a masked
//      copy back (gf2_mul_dev writes no destination that aliases an operand); an update is an accumulate product of a panel of T
//      with the solved part of B.  All products go through gf2_mul_dev on windows; split points are multiples of d.
// Only B's bits under the word masks change: windows of dirty parents stay intact, excess bits of a gf2_dmat stay zero.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "dev_args.h"
#include "gf2_kernels.h"

typedef uint64_t u64;

namespace {

constexpr int TRSM_BLOCK = 512;  // d: the fastest of 64 / 128 / 256 / 512 at every size measured

__device__ __forceinline__ u64 rdlane(u64 v, int lane) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 low_bits(int n) { return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1)); }

// acc ^= XOR of val[b * stride] over the set bits b of `bits` (val: LDS, the same address in every lane)
__device__ __forceinline__ u64 select_xor(u64 acc, u64 bits, const u64 *val, int stride) {
#pragma unroll 16
  for (int b = 0; b < 64; ++b) acc ^= (0ull - ((bits >> b) & 1)) & val[b * stride];
  return acc;
}

// Block j = rows and columns [j * d, j * d + d) of the n x n matrix T (unit lower or upper triangular; ragged last block completed
// with the identity) -> its inverse at inv + j * d * ldi, d / 64 words per row.  d = 64, 128, 256 or 512 = blockDim.x; dynamic LDS:
// 2 * d * (d / 64) words (S: the clean triangle, later the half products; V: the inverse).
template <bool UPPER>
__global__ void __launch_bounds__(512) trsm_invert_blocks(const u64 *T, long long ldt, int n, int d, u64 *inv, long long ldi) {
  extern __shared__ u64 trsm_lds[];
  const int dw = d >> 6;
  u64 *S = trsm_lds, *V = trsm_lds + d * dw;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * d;
  const int nr = min(d, n - r0);
  const u64 *Tb = T + (long long)r0 * ldt + (r0 >> 6);
  for (int t = tid; t < d * dw; t += d) {
    const int r = t / dw, q = t - r * dw;
    u64 v = 0;
    if (r < nr) {
      const int lo = r - q * 64;  // bits of this word left of the diagonal
      const u64 m = UPPER ? (~low_bits(lo + 1) & low_bits(nr - q * 64)) : low_bits(lo);
      if (m) v = Tb[(long long)r * ldt + q] & m;  // m != 0: column q * 64 lies inside the block's nr columns
    }
    S[t] = v;
    V[t] = 0;
  }
  __syncthreads();
  {  // wave wv: the 64 x 64 diagonal sub-block wv, row tid in lane `lane`
    const u64 t = S[tid * dw + wv];
    u64 x = 1ull << lane;
    if (!UPPER) {
#pragma unroll
      for (int k = 0; k < 63; ++k) {
        const u64 xk = rdlane(x, k);  // row k is final: its own bits are all below k
        if ((t >> k) & 1) x ^= xk;
      }
    } else {
#pragma unroll
      for (int k = 63; k > 0; --k) {
        const u64 xk = rdlane(x, k);
        if ((t >> k) & 1) x ^= xk;
      }
    }
    V[tid * dw + wv] = x;
  }
  __syncthreads();
  // doubling: diagonal blocks of h rows at p (first) and p + h (second); X = the off-diagonal block: rows rx, columns cx
  for (int h = 64; h < d; h <<= 1) {
    const int hw = h >> 6;
    const int items = (d / (2 * h)) * hw * hw;  // (pair, row group g, word w): one wave each, <= 2 per wave
    u64 acc[2] = {0, 0};
    // phase 1: W = X * inv(diagonal block at cx), kept in registers until every wave has read X
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int it = wv + c * dw;
      if (it >= items) break;
      const int pair = it / (hw * hw), g = (it / hw) % hw, w = it % hw;
      const int p = pair * 2 * h, rx = UPPER ? p : p + h, cx = UPPER ? p + h : p;
      const u64 *bits = S + (rx + g * 64 + lane) * dw + (cx >> 6);
      const u64 *val = V + cx * dw + (cx >> 6) + w;
      u64 a = 0;
      // word w of row k of a triangular inverse is zero for k / 64 < w (lower) or k / 64 > w (upper)
      for (int kw = UPPER ? 0 : w; kw < (UPPER ? w + 1 : hw); ++kw) a = select_xor(a, bits[kw], val + kw * 64 * dw, dw);
      acc[c] = a;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int it = wv + c * dw;
      if (it >= items) break;
      const int pair = it / (hw * hw), g = (it / hw) % hw, w = it % hw;
      const int p = pair * 2 * h, rx = UPPER ? p : p + h, cx = UPPER ? p + h : p;
      S[(rx + g * 64 + lane) * dw + (cx >> 6) + w] = acc[c];
    }
    __syncthreads();
    // phase 2: inverse's off-diagonal block = inv(diagonal block at rx) * W
    for (int it = wv; it < items; it += dw) {
      const int pair = it / (hw * hw), g = (it / hw) % hw, w = it % hw;
      const int p = pair * 2 * h, rx = UPPER ? p : p + h, cx = UPPER ? p + h : p;
      const u64 *bits = V + (rx + g * 64 + lane) * dw + (rx >> 6);
      const u64 *val = S + rx * dw + (cx >> 6) + w;
      u64 a = 0;
      // word kw of row g * 64 + lane of a triangular inverse is zero for kw > g (lower) or kw < g (upper)
      for (int kw = UPPER ? g : 0; kw < (UPPER ? hw : g + 1); ++kw) a = select_xor(a, bits[kw], val + kw * 64 * dw, dw);
      V[(rx + g * 64 + lane) * dw + (cx >> 6) + w] = a;
    }
    __syncthreads();
  }
  u64 *out = inv + (long long)blockIdx.x * d * ldi;
  for (int t = tid; t < d * dw; t += d) {
    const int r = t / dw, q = t - r * dw;
    out[(long long)r * ldi + q] = V[t];
  }
}

// dst[i][w] = src[i][w] for w < words, the last word only under lastmask (a leaf's result from scratch into its block of B)
__global__ void __launch_bounds__(256) trsm_copy_back(u64 *dst, long long ldd, const u64 *src, long long lds_, int rows, int words,
                                                      u64 lastmask) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)rows * words) return;
  const int i = (int)(t / words), w = (int)(t % words);
  const u64 v = src[(long long)i * lds_ + w];
  u64 *p = dst + (long long)i * ldd + w;
  *p = w == words - 1 ? ((*p & ~lastmask) | (v & lastmask)) : v;
}

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------

inline int words_of(long long bits) { return (int)((bits + 63) >> 6); }
inline u64 last_mask(long long bits) { return (bits & 63) ? ((1ull << (bits & 63)) - 1) : ~0ull; }
inline long long even_ld(long long w) { return (w + 1) & ~1ll; }


inline gf2_dmat win(const gf2_dmat &A, long long r, long long c, int rows, int cols) {  // c: multiple of 64
  return gf2_dmat{static_cast<u64 *>(A.data) + r * A.ld + (c >> 6), A.ld, rows, cols};
}

// block size of the diagonal inversion for an n x n solve: TRSM_BLOCK (M4RI_HIP_TRSM_BLOCK = 64 | 128 | 256 | 512 overrides it:
// tools/trsm_bench.py, tests), but no larger than the smallest of the four that holds all of T (a workgroup sized to the block)
int trsm_block(int n) {
  const char *e = std::getenv("M4RI_HIP_TRSM_BLOCK");  // read per call: tests switch it
  const int v = e ? std::atoi(e) : 0;
  int d = (v == 64 || v == 128 || v == 256 || v == 512) ? v : TRSM_BLOCK;
  while (d > 64 && d / 2 >= n) d /= 2;
  return d;
}

struct TrsmCtx {
  gf2_dmat T, B;
  int n, d;
  bool upper, right;
  u64 *inv;       // ceil(n / d) blocks of d rows, ldi words each
  long long ldi;
  u64 *tmp;       // a leaf's result: d x ldt (left) or B.nrows x ldt (right) words
  long long ldt;
  hipStream_t s;
};

int leaf(const TrsmCtx &c, int b) {
  const int r = b * c.d, nr = std::min(c.d, c.n - r);
  gf2_dmat I{c.inv + (long long)b * c.d * c.ldi, c.ldi, nr, nr};
  gf2_dmat X = c.right ? win(c.B, 0, r, c.B.nrows, nr) : win(c.B, r, 0, nr, c.B.ncols);
  gf2_dmat S{c.tmp, c.ldt, X.nrows, X.ncols};
  GF2_RC(c.right ? gf2_mul_dev(&S, &X, &I, 0, 0, 0, c.s) : gf2_mul_dev(&S, &I, &X, 0, 0, 0, c.s));
  const int words = words_of(X.ncols);
  hipLaunchKernelGGL(trsm_copy_back, dim3((unsigned)(((long long)X.nrows * words + 255) / 256)), dim3(256), 0, c.s,
                     static_cast<u64 *>(X.data), X.ld, c.tmp, c.ldt, X.nrows, words, last_mask(X.ncols));
  HIP_TRY(hipGetLastError());
  return 0;
}

// blocks [b0, b1) of the diagonal
int solve(const TrsmCtx &c, int b0, int b1) {
  if (b1 - b0 == 1) return leaf(c, b0);
  const int mid = b0 + (b1 - b0 + 1) / 2;
  const int r = b0 * c.d, rm = mid * c.d, h1 = rm - r, h2 = std::min(c.n, b1 * c.d) - rm;
  // the half solved first: the one no other block of the triangle feeds into
  const bool first_low = c.right ? c.upper : !c.upper;
  GF2_RC(first_low ? solve(c, b0, mid) : solve(c, mid, b1));
  if (!c.right) {
    const int k = c.B.ncols;
    if (first_low) {  // B2 ^= T21 X1
      gf2_dmat C = win(c.B, rm, 0, h2, k), A = win(c.T, rm, r, h2, h1), X = win(c.B, r, 0, h1, k);
      GF2_RC(gf2_mul_dev(&C, &A, &X, 1, 0, 0, c.s));
    } else {  // B1 ^= T12 X2
      gf2_dmat C = win(c.B, r, 0, h1, k), A = win(c.T, r, rm, h1, h2), X = win(c.B, rm, 0, h2, k);
      GF2_RC(gf2_mul_dev(&C, &A, &X, 1, 0, 0, c.s));
    }
  } else {
    const int k = c.B.nrows;
    if (first_low) {  // B2 ^= X1 T12
      gf2_dmat C = win(c.B, 0, rm, k, h2), X = win(c.B, 0, r, k, h1), A = win(c.T, r, rm, h1, h2);
      GF2_RC(gf2_mul_dev(&C, &X, &A, 1, 0, 0, c.s));
    } else {  // B1 ^= X2 T21
      gf2_dmat C = win(c.B, 0, r, k, h1), X = win(c.B, 0, rm, k, h2), A = win(c.T, rm, r, h2, h1);
      GF2_RC(gf2_mul_dev(&C, &X, &A, 1, 0, 0, c.s));
    }
  }
  return first_low ? solve(c, mid, b1) : solve(c, b0, mid);
}

// the scratch of a call lives in the stream's arena from the first launch to the last: calls on one stream from several host
// threads must not interleave
std::mutex g_trsm_mu;

}  // namespace

extern "C" int gf2_trsm_dev(gf2_dmat const *T, gf2_dmat *B, int upper, int right, void *stream) {
  static const char fn[] = "gf2_trsm_dev";
  if (gf2_check_mat(fn, "T", T) || gf2_check_mat(fn, "B", B)) return -1;
  if (T->nrows != T->ncols) return gf2_bad_arg(fn, "T is not square");
  if ((right ? B->ncols : B->nrows) != T->nrows) return gf2_bad_arg(fn, "dimension mismatch");
  const int n = T->nrows;
  if (n == 0 || B->nrows == 0 || B->ncols == 0) return 0;
  if (int rc = gf2_refuse_overlap(fn, "B", B, "T", T)) return rc;  // blocks of B are rewritten while later steps still read T
  GF2_RC(gf2_require_device_for(fn));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int d = trsm_block(n), nb = (n + d - 1) / d;
  TrsmCtx c{*T, *B, n, d, upper != 0, right != 0, nullptr, even_ld(d >> 6), nullptr, 0, s};
  c.ldt = even_ld(right ? d >> 6 : words_of(B->ncols));
  const size_t tmp_rows = right ? (size_t)B->nrows : (size_t)d;
  std::lock_guard<std::mutex> lk(g_trsm_mu);
  void *p = nullptr;
  GF2_RC(gf2_stream_scratch(s, (size_t)nb * d * c.ldi * 8, &p, GF2_SLOT_TRSM_INVERSES));
  c.inv = static_cast<u64 *>(p);
  GF2_RC(gf2_stream_scratch(s, tmp_rows * c.ldt * 8, &p, GF2_SLOT_TRSM_LEAF));
  c.tmp = static_cast<u64 *>(p);
  const size_t lds_bytes = (size_t)2 * d * (d >> 6) * 8;  // 64 KiB at d = 512
  if (upper)
    hipLaunchKernelGGL(trsm_invert_blocks<true>, dim3(nb), dim3(d), lds_bytes, s, static_cast<const u64 *>(T->data), (long long)T->ld, n,
                       d, c.inv, c.ldi);
  else
    hipLaunchKernelGGL(trsm_invert_blocks<false>, dim3(nb), dim3(d), lds_bytes, s, static_cast<const u64 *>(T->data), (long long)T->ld, n,
                       d, c.inv, c.ldi);
  HIP_TRY(hipGetLastError());
  return solve(c, 0, nb);
}
