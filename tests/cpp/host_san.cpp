// host_san.cpp -- the host units of the library (mzd_host, gf2_small_host, ple_host, trsm_host, nullspace_host) under the host compiler's
// address and undefined-behaviour sanitizers, stand-alone: tests/test_host_sanitized.py links them with this file, host_san_stubs.cpp
// and the C oracle (the reference here; a test binary, the product never links it).  These routines run inside the caller's process,
// on its heap through rows[] and on windows of its matrices; through ctypes no sanitizer can watch them.
//
// Every case runs on a plain matrix and on a window at (3, 64) of a dirty parent whose columns do not end on a word.  Every result is
// compared bit for bit with the oracle or with a plain loop written here, and the parent -- for a plain matrix: the excess bits of the
// last word and the padding words of the row stride -- is compared bit by bit outside the operand.  Leak detection is on: a matrix that
// a routine forgets to free fails the run.  The overlap predicates of dev_args.h are pure arithmetic and run here too, against
// enumerated bits and bytes.  argv[1]: a directory for the file of the save / load round trip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "dev_args.h"
#include "gf2_oracle.h"

extern int g_stub_devices, g_stub_device_calls, g_stub_pin_requests;
typedef uint64_t u64;
static std::mt19937_64 rng(777);
static const int DIMS[] = {1, 2, 63, 64, 65, 100, 127, 128, 129, 191, 200};
static const int NDIMS = 11;

#define FAIL(...)                    \
  do {                               \
    printf("MISMATCH " __VA_ARGS__); \
    printf("\n");                    \
    exit(1);                         \
  } while (0)

static int wordsof(int bits) { return (bits + 63) / 64; }
static u64 lastmask(int bits) { return (bits & 63) ? ((1ull << (bits & 63)) - 1) : ~0ull; }
static int getbit(const u64 *row, int c) { return (int)((row[c >> 6] >> (c & 63)) & 1); }
static void setbit(u64 *row, int c, int v) { row[c >> 6] = (row[c >> 6] & ~(1ull << (c & 63))) | ((u64)(v & 1) << (c & 63)); }
typedef std::vector<u64> Dense;  // r rows of wordsof(c) words, excess bits zero

static Dense random_dense(int r, int c) {
  const int w = wordsof(c);
  Dense d((size_t)r * w);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < w; ++j) d[(size_t)i * w + j] = rng() & (j == w - 1 ? lastmask(c) : ~0ull);
  return d;
}
// kind 0: zero, 1: rank one, 2: rank about min(r, c) / 2, 3: random
static Dense dense_of_kind(int r, int c, int kind) {
  const int w = wordsof(c);
  if (kind == 3) return random_dense(r, c);
  Dense d((size_t)r * w, 0);
  if (kind == 0) return d;
  const int k = kind == 1 ? 1 : std::max(1, std::min(r, c) / 2);
  Dense X = random_dense(r, k), Y = random_dense(k, c);
  if (kind == 1) X[rng() % r] |= 1, Y[0] |= 1;  // neither factor is zero
  for (int i = 0; i < r; ++i)
    for (int t = 0; t < k; ++t)
      if (getbit(&X[(size_t)i * wordsof(k)], t))
        for (int j = 0; j < w; ++j) d[(size_t)i * w + j] ^= Y[(size_t)t * w + j];
  return d;
}

// a matrix under test: plain, or a window at (3, 64) of a dirty parent
struct Mat {
  mzd_t *parent = nullptr, *m = nullptr;
  int r0 = 0, c0 = 0;
  std::vector<u64> before;  // the raw block of the parent (of m itself for a plain matrix), whole row strides
  mzd_t *top() const { return parent ? parent : m; }
};
static void put(Mat &M, const Dense &d) {
  const int w = M.m->width;
  for (int i = 0; i < M.m->nrows; ++i)
    for (int j = 0; j < w; ++j) {
      u64 &x = M.m->rows[i][j];
      x = j == w - 1 ? ((x & ~M.m->high_bitmask) | (d[(size_t)i * w + j] & M.m->high_bitmask)) : d[(size_t)i * w + j];
    }
}
static void seal(Mat &M) {
  const mzd_t *t = M.top();
  M.before.assign((size_t)t->nrows * t->rowstride, 0);
  for (int i = 0; i < t->nrows; ++i) memcpy(&M.before[(size_t)i * t->rowstride], t->rows[i], (size_t)t->rowstride * 8);
}
static Mat make(int r, int c, bool window, const Dense *content = nullptr) {
  Mat M;
  if (window) {
    const int extra = (c + 37) % 64 ? 37 : 38;
    M.parent = mzd_init(r + 5, 64 + c + extra);
    for (int i = 0; i < M.parent->nrows; ++i)
      for (int j = 0; j < M.parent->width; ++j) M.parent->rows[i][j] = rng() & (j == M.parent->width - 1 ? M.parent->high_bitmask : ~0ull);
    M.r0 = 3, M.c0 = 64;
    M.m = mzd_init_window(M.parent, 3, 64, 3 + r, 64 + c);
  } else {
    M.m = mzd_init(r, c);
  }
  if (M.m->nrows != r || M.m->ncols != c || M.m->width != wordsof(c)) FAIL("make: shape");
  put(M, content ? *content : random_dense(r, c));
  seal(M);
  return M;
}
static void release(Mat &M) {
  mzd_free(M.m);
  if (M.parent) mzd_free(M.parent);
  M.m = M.parent = nullptr;
}
static Dense dense(const mzd_t *A) {
  const int w = wordsof(A->ncols);
  Dense d((size_t)A->nrows * w);
  for (int i = 0; i < A->nrows; ++i)
    for (int j = 0; j < w; ++j) d[(size_t)i * w + j] = A->rows[i][j] & (j == w - 1 ? lastmask(A->ncols) : ~0ull);
  return d;
}
// no bit outside the operand changed: the parent's other rows and columns, excess bits, padding words
static void outside(const Mat &M, const char *what, int a, int b) {
  const mzd_t *t = M.top();
  for (int i = 0; i < t->nrows; ++i)
    for (int q = 0; q < t->rowstride; ++q) {
      u64 inside = 0;
      if (i >= M.r0 && i < M.r0 + M.m->nrows)
        for (int bit = 0; bit < 64; ++bit) {
          const int col = q * 64 + bit;
          if (col >= M.c0 && col < M.c0 + M.m->ncols) inside |= 1ull << bit;
        }
      if ((t->rows[i][q] ^ M.before[(size_t)i * t->rowstride + q]) & ~inside)
        FAIL("%s (%d x %d, %s): a bit outside the operand changed, parent row %d word %d", what, a, b, M.parent ? "window" : "plain", i, q);
    }
}
static void expect(const Mat &M, const Dense &want, const char *what, int a, int b, int x = 0) {
  const Dense got = dense(M.m);
  if (got.size() != want.size()) FAIL("%s: size", what);
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i] != want[i])
      FAIL("%s (%d x %d, %s, %d): word %zu is %016llx, want %016llx", what, a, b, M.parent ? "window" : "plain", x, i,
           (unsigned long long)got[i], (unsigned long long)want[i]);
  outside(M, what, a, b);
}
static void unchanged(const Mat &M, const char *what, int a, int b) {
  const mzd_t *t = M.top();
  for (int i = 0; i < t->nrows; ++i)
    if (memcmp(t->rows[i], &M.before[(size_t)i * t->rowstride], (size_t)t->rowstride * 8)) FAIL("%s (%d x %d): a source operand changed", what, a, b);
}
static void report(const char *name, long n) {
  if (g_stub_device_calls) FAIL("%s: %d calls left the host routines for a device entry", name, g_stub_device_calls);
  printf("%s: %ld cases ok\n", name, n);
  fflush(stdout);
}
#define FOR_SHAPES for (int r : DIMS) for (int c : DIMS) for (int win = 0; win < 2; ++win)

// ---------------------------------------------------------------------------------------------------------------------------------
static void run_echelonize() {
  long n1 = 0, n0 = 0;
  FOR_SHAPES for (int kind = 0; kind < 4; ++kind) {
    const int w = wordsof(c);
    const Dense d = dense_of_kind(r, c, kind);
    Dense ref = d;
    std::vector<int> piv(std::min(r, c));
    const int rank = oracle_echelonize(ref.data(), w, r, c, 0, 1, piv.data());
    if ((kind == 0 && rank != 0) || (kind == 1 && rank != 1)) FAIL("echelonize driver: rank of the input");
    Mat A = make(r, c, win, &d);
    if (gf2_echelonize_host_small(A.m, 1) != rank) FAIL("echelonize full rank %d x %d kind %d", r, c, kind);
    expect(A, ref, "gf2_echelonize_host_small full", r, c, kind);
    release(A);
    ++n1;
    // full = 0: rank, pivot columns, zero rows below, and the same reduced form after re-reduction
    Mat B = make(r, c, win, &d);
    if (gf2_echelonize_host_small(B.m, 0) != rank) FAIL("echelonize rank %d x %d kind %d", r, c, kind);
    Dense g = dense(B.m);
    outside(B, "gf2_echelonize_host_small", r, c);
    for (int i = 0; i < r; ++i) {
      int first = -1;
      for (int j = 0; j < c && first < 0; ++j)
        if (getbit(&g[(size_t)i * w], j)) first = j;
      if (first != (i < rank ? piv[i] : -1)) FAIL("echelonize %d x %d kind %d: row %d starts at %d", r, c, kind, i, first);
    }
    if (oracle_echelonize(g.data(), w, r, c, 0, 1, nullptr) != rank || g != ref) FAIL("echelonize %d x %d kind %d: another row space", r, c, kind);
    release(B);
    ++n0;
  }
  report("gf2_echelonize_host_small full", n1);
  report("gf2_echelonize_host_small", n0);
}

static void run_ple() {
  long n = 0;
  FOR_SHAPES for (int kind = 2; kind < 4; ++kind) for (int pluq = 0; pluq < 2; ++pluq) {
    const int w = wordsof(c);
    const Dense d = dense_of_kind(r, c, kind);
    Dense ref = d;
    std::vector<int> P(r), Q(c), P2(r, -1), Q2(c, -1);
    const int rank = oracle_ple(ref.data(), w, r, c, pluq, P.data(), Q.data());
    Mat A = make(r, c, win, &d);
    if (gf2_ple_host_small(A.m, pluq, P2.data(), Q2.data()) != rank) FAIL("ple rank %d x %d", r, c);
    expect(A, ref, pluq ? "gf2_ple_host_small pluq" : "gf2_ple_host_small ple", r, c, kind);
    if (P != P2 || Q != Q2) FAIL("ple %d x %d kind %d pluq %d: P or Q", r, c, kind, pluq);
    release(A);
    ++n;
  }
  report("gf2_ple_host_small", n);
}

// T X = B (left) or X T = B (right), T unit triangular with anything on the diagonal and in the other triangle
static void run_trsm() {
  long n = 0;
  for (int nn : DIMS) for (int k : DIMS) for (int win = 0; win < 2; ++win) for (int v = 0; v < 4; ++v) {
    const int upper = v & 1, right = v >> 1, br = right ? k : nn, bc = right ? nn : k, bw = wordsof(bc), tw = wordsof(nn);
    const Dense t = random_dense(nn, nn), b = random_dense(br, bc);
    auto tri = [&](int i, int j) { return (upper ? j > i : j < i) ? getbit(&t[(size_t)i * tw], j) : 0; };
    Dense tcol((size_t)nn * tw, 0);  // column j of the strict triangle as a row of bits
    for (int i = 0; i < nn; ++i)
      for (int j = 0; j < nn; ++j) setbit(&tcol[(size_t)j * tw], i, tri(i, j));
    Dense x = b;
    if (!right) {
      for (int s = 0; s < nn; ++s) {
        const int i = upper ? nn - 1 - s : s;  // row i of X = row i of B + the rows of X that T's row i names
        for (int j = 0; j < nn; ++j)
          if (tri(i, j))
            for (int q = 0; q < bw; ++q) x[(size_t)i * bw + q] ^= x[(size_t)j * bw + q];
      }
    } else {
      for (int row = 0; row < br; ++row)
        for (int s = 0; s < nn; ++s) {
          const int j = upper ? s : nn - 1 - s;  // X[row][j] = B[row][j] + sum over i of X[row][i] T[i][j]
          int bit = getbit(&x[(size_t)row * bw], j);
          for (int q = 0; q < tw; ++q) bit ^= __builtin_parityll(x[(size_t)row * bw + q] & tcol[(size_t)j * tw + q]);  // bw == tw
          setbit(&x[(size_t)row * bw], j, bit);
        }
    }
    Mat T = make(nn, nn, win, &t), B = make(br, bc, win, &b);
    if (gf2_trsm_host_small(T.m, B.m, upper, right) != 0) FAIL("trsm status");
    expect(B, x, "gf2_trsm_host_small", nn, k, v);
    unchanged(T, "gf2_trsm_host_small", nn, k);
    release(T), release(B);
    ++n;
  }
  report("gf2_trsm_host_small", n);
}

static void run_nullspace() {
  long n = 0;
  FOR_SHAPES for (int kind = 0; kind < 4; ++kind) {
    const int w = wordsof(c);
    const Dense d = dense_of_kind(r, c, kind);
    Dense ref = d;
    std::vector<int> piv(std::min(r, c));
    const int rank = oracle_echelonize(ref.data(), w, r, c, 0, 1, piv.data()), dd = c - rank, kw = wordsof(dd);
    Mat A = make(r, c, win, &d);
    mzd_t *K = nullptr;
    if (gf2_nullspace_host_small(A.m, &K) != rank) FAIL("nullspace rank %d x %d kind %d", r, c, kind);
    expect(A, ref, "gf2_nullspace_host_small", r, c, kind);
    if ((K == nullptr) != (dd == 0)) FAIL("nullspace %d x %d kind %d: K", r, c, kind);
    if (K) {
      if (K->nrows != c || K->ncols != dd) FAIL("nullspace %d x %d: shape of K", r, c);
      std::vector<char> isp(c, 0);
      for (int i = 0; i < rank; ++i) isp[piv[i]] = 1;
      std::vector<int> fr;
      for (int j = 0; j < c; ++j)
        if (!isp[j]) fr.push_back(j);
      Dense want((size_t)c * kw, 0);  // row f_j = e_j, row p_i = E's row i at the free columns
      for (int j = 0; j < dd; ++j) setbit(&want[(size_t)fr[j] * kw], j, 1);
      for (int i = 0; i < rank; ++i)
        for (int j = 0; j < dd; ++j) setbit(&want[(size_t)piv[i] * kw], j, getbit(&ref[(size_t)i * w], fr[j]));
      for (int i = 0; i < c; ++i)
        for (int q = 0; q < kw; ++q)
          if (K->rows[i][q] != want[(size_t)i * kw + q]) FAIL("nullspace %d x %d kind %d: K row %d word %d", r, c, kind, i, q);  // excess bits zero
      mzd_free(K);
    }
    release(A);
    ++n;
  }
  report("gf2_nullspace_host_small", n);
}

static void run_mul() {
  long n = 0, nt = 0;
  int pick = 0;
  FOR_SHAPES for (int rep = 0; rep < 2; ++rep) for (int acc = 0; acc < 2; ++acc) {
    const int l = DIMS[(pick += 3 + rep) % NDIMS], w = wordsof(c);
    const Dense a = random_dense(r, l), b = random_dense(l, c), c0 = random_dense(r, c);
    Dense want(c0.size(), 0);
    oracle_mul_naive(want.data(), w, a.data(), wordsof(l), b.data(), w, r, l, c);
    if (acc)
      for (size_t i = 0; i < want.size(); ++i) want[i] ^= c0[i];
    {
      Mat A = make(r, l, win, &a), B = make(l, c, win, &b), C = make(r, c, win, &c0);
      if (gf2_mul_host_small(C.m, A.m, B.m, acc) != 0) FAIL("mul status");
      expect(C, want, "gf2_mul_host_small", r, c, l);
      unchanged(A, "gf2_mul_host_small", r, c), unchanged(B, "gf2_mul_host_small", r, c);
      release(A), release(B), release(C);
      ++n;
    }
    {
      Dense bt((size_t)c * wordsof(l), 0);
      for (int i = 0; i < l; ++i)
        for (int j = 0; j < c; ++j) setbit(&bt[(size_t)j * wordsof(l)], i, getbit(&b[(size_t)i * w], j));
      Mat A = make(r, l, win, &a), Bt = make(c, l, win, &bt), C = make(r, c, win, &c0);
      if (gf2_mul_nt_host_small(C.m, A.m, Bt.m, acc) != 0) FAIL("mul_nt status");
      expect(C, want, "gf2_mul_nt_host_small", r, c, l);
      unchanged(A, "gf2_mul_nt_host_small", r, c), unchanged(Bt, "gf2_mul_nt_host_small", r, c);
      release(A), release(Bt), release(C);
      ++nt;
    }
  }
  report("gf2_mul_host_small", n);
  report("gf2_mul_nt_host_small", nt);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the containers of mzd_host.cpp
// ---------------------------------------------------------------------------------------------------------------------------------
static void run_containers(const std::string &dir) {
  long n_win = 0, n_copy = 0, n_tr = 0, n_add = 0, n_cat = 0, n_stack = 0, n_sub = 0, n_rows = 0, n_cols = 0, n_clear = 0, n_pred = 0, n_ui = 0,
       n_tab = 0, n_inv = 0, n_perm = 0, n_file = 0;
  int pick = 0;
  FOR_SHAPES {
    const int w = wordsof(c), c2 = DIMS[(pick += 5) % NDIMS], r2 = DIMS[(pick + 3) % NDIMS];
    const Dense a = random_dense(r, c), b = random_dense(r, c);
    {  // mzd_init_window: the window's rows are the parent's; a window of the window
      Mat A = make(r, c, win, &a);
      if (dense(A.m) != a) FAIL("mzd_init_window %d x %d", r, c);
      const int lr = r / 2, hr = r, lc = c > 64 ? 64 : 0, hc = c;
      mzd_t *W = mzd_init_window(A.m, lr, lc, hr, hc);
      for (int i = 0; i < hr - lr; ++i)
        for (int j = 0; j < hc - lc; ++j)
          if (getbit(W->rows[i], j) != getbit(&a[(size_t)(lr + i) * w], lc + j)) FAIL("mzd_init_window of a window %d x %d", r, c);
      mzd_free(W);
      unchanged(A, "mzd_init_window", r, c);
      release(A);
      ++n_win;
    }
    for (int given = 0; given < 2; ++given) {  // mzd_copy, mzd_transpose: into a given matrix, into a fresh one
      Mat A = make(r, c, win, &a), N = make(r, c, win), D = make(c, r, win);
      mzd_t *got = mzd_copy(given ? N.m : nullptr, A.m);
      if (given ? got != N.m : got == nullptr) FAIL("mzd_copy result");
      if (given) expect(N, a, "mzd_copy", r, c);
      else if (dense(got) != a || !mzd_equal(got, A.m)) FAIL("mzd_copy fresh %d x %d", r, c);
      if (!given) mzd_free(got);
      Dense t((size_t)c * wordsof(r), 0);
      for (int i = 0; i < r; ++i)
        for (int j = 0; j < c; ++j) setbit(&t[(size_t)j * wordsof(r)], i, getbit(&a[(size_t)i * w], j));
      got = mzd_transpose(given ? D.m : nullptr, A.m);
      if (given) expect(D, t, "mzd_transpose", r, c);
      else if (dense(got) != t) FAIL("mzd_transpose fresh %d x %d", r, c);
      if (!given) mzd_free(got);
      unchanged(A, "mzd_copy / mzd_transpose", r, c);
      release(A), release(N), release(D);
      ++n_copy, ++n_tr;
    }
    for (int mode = 0; mode < 3; ++mode) {  // mzd_add: into a third matrix, in place, fresh; mzd_sub is the same sum
      Mat A = make(r, c, win, &a), B = make(r, c, win, &b), C = make(r, c, win);
      Dense s = a;
      for (size_t i = 0; i < s.size(); ++i) s[i] ^= b[i];
      mzd_t *got = mode == 0 ? mzd_add(C.m, A.m, B.m) : mode == 1 ? mzd_sub(A.m, A.m, B.m) : mzd_add(nullptr, A.m, B.m);
      if (mode == 0) expect(C, s, "mzd_add", r, c);
      else if (mode == 1) expect(A, s, "mzd_sub in place", r, c);
      else if (dense(got) != s) FAIL("mzd_add fresh %d x %d", r, c);
      if (mode == 2) mzd_free(got);
      if (mode != 1) unchanged(A, "mzd_add", r, c);
      unchanged(B, "mzd_add", r, c);
      release(A), release(B), release(C);
      ++n_add;
    }
    for (int given = 0; given < 2; ++given) {  // mzd_concat, mzd_stack, mzd_submatrix
      const Dense bc = random_dense(r, c2), bs = random_dense(r2, c);
      Mat A = make(r, c, win, &a), B = make(r, c2, win, &bc), C = make(r, c + c2, win), S = make(r2, c, win, &bs), T = make(r + r2, c, win);
      Dense cat((size_t)r * wordsof(c + c2), 0), st((size_t)(r + r2) * w, 0);
      for (int i = 0; i < r; ++i) {
        for (int j = 0; j < c; ++j) setbit(&cat[(size_t)i * wordsof(c + c2)], j, getbit(&a[(size_t)i * w], j));
        for (int j = 0; j < c2; ++j) setbit(&cat[(size_t)i * wordsof(c + c2)], c + j, getbit(&bc[(size_t)i * wordsof(c2)], j));
      }
      std::copy(a.begin(), a.end(), st.begin());
      std::copy(bs.begin(), bs.end(), st.begin() + (long)a.size());
      mzd_t *got = mzd_concat(given ? C.m : nullptr, A.m, B.m);
      if (given) expect(C, cat, "mzd_concat", r, c, c2);
      else if (dense(got) != cat) FAIL("mzd_concat fresh %d x %d + %d", r, c, c2);
      if (!given) mzd_free(got);
      got = mzd_stack(given ? T.m : nullptr, A.m, S.m);
      if (given) expect(T, st, "mzd_stack", r, c, r2);
      else if (dense(got) != st) FAIL("mzd_stack fresh %d + %d x %d", r, r2, c);
      if (!given) mzd_free(got);
      const int lr = (int)(rng() % r), hr = lr + 1 + (int)(rng() % (r - lr)), lc = (int)(rng() % c), hc = lc + 1 + (int)(rng() % (c - lc));
      Dense sub((size_t)(hr - lr) * wordsof(hc - lc), 0);
      for (int i = lr; i < hr; ++i)
        for (int j = lc; j < hc; ++j) setbit(&sub[(size_t)(i - lr) * wordsof(hc - lc)], j - lc, getbit(&a[(size_t)i * w], j));
      Mat U = make(hr - lr, hc - lc, win);
      got = mzd_submatrix(given ? U.m : nullptr, A.m, lr, lc, hr, hc);
      if (given) expect(U, sub, "mzd_submatrix", r, c);
      else if (dense(got) != sub) FAIL("mzd_submatrix fresh %d x %d", r, c);
      if (!given) mzd_free(got);
      unchanged(A, "mzd_concat / mzd_stack / mzd_submatrix", r, c), unchanged(B, "mzd_concat", r, c), unchanged(S, "mzd_stack", r, c);
      release(A), release(B), release(C), release(S), release(T), release(U);
      ++n_cat, ++n_stack, ++n_sub;
    }
    {  // mzd_row_swap, mzd_copy_row
      Mat A = make(r, c, win, &a), B = make(r, c, win, &b);
      const int x = (int)(rng() % r), y = (int)(rng() % r);
      Dense s = a;
      for (int j = 0; j < w; ++j) std::swap(s[(size_t)x * w + j], s[(size_t)y * w + j]);
      mzd_row_swap(A.m, x, y);
      expect(A, s, "mzd_row_swap", r, c);
      Dense t = b;
      for (int j = 0; j < w; ++j) t[(size_t)x * w + j] = s[(size_t)y * w + j];
      mzd_copy_row(B.m, x, A.m, y);
      expect(B, t, "mzd_copy_row", r, c);
      release(A), release(B);
      ++n_rows;
    }
    {  // mzd_col_swap: the first, the last, two of one word, two random ones
      const int pairs[][2] = {{0, c - 1}, {c - 1, c - 1}, {(c - 1) / 64 * 64, c - 1}, {(int)(rng() % c), (int)(rng() % c)}};
      for (const auto &p : pairs) {
        Mat A = make(r, c, win, &a);
        Dense s = a;
        for (int i = 0; i < r; ++i) {
          const int x = getbit(&a[(size_t)i * w], p[0]), y = getbit(&a[(size_t)i * w], p[1]);
          setbit(&s[(size_t)i * w], p[0], y), setbit(&s[(size_t)i * w], p[1], x);
        }
        mzd_col_swap(A.m, p[0], p[1]);
        expect(A, s, "mzd_col_swap", r, c);
        release(A);
        ++n_cols;
      }
    }
    for (int off : {0, 1, c / 2, c - 1, c, c / 64 * 64, 63 < c ? 63 : 0}) {  // mzd_row_clear_offset
      Mat A = make(r, c, win, &a);
      const int row = (int)(rng() % r);
      Dense s = a;
      for (int j = off; j < c; ++j) setbit(&s[(size_t)row * w], j, 0);
      mzd_row_clear_offset(A.m, row, off);
      expect(A, s, "mzd_row_clear_offset", r, c, off);
      release(A);
      ++n_clear;
    }
    {  // mzd_is_zero, mzd_equal: only bits of the operand count (a window's last word carries its parent's bits)
      const Dense z((size_t)r * w, 0);
      Mat Z = make(r, c, win, &z), A = make(r, c, win, &a), A2 = make(r, c, !win, &a);
      if (!mzd_is_zero(Z.m)) FAIL("mzd_is_zero of zero %d x %d", r, c);
      if (!mzd_equal(A.m, A2.m) || !mzd_equal(A.m, A.m)) FAIL("mzd_equal of equals %d x %d", r, c);
      Dense one = z;
      setbit(&one[(size_t)(r - 1) * w], c - 1, 1);  // the last bit of the last row
      put(Z, one);
      if (mzd_is_zero(Z.m)) FAIL("mzd_is_zero misses the last bit %d x %d", r, c);
      Dense a1 = a;
      setbit(&a1[(size_t)(r - 1) * w], c - 1, !getbit(&a[(size_t)(r - 1) * w], c - 1));
      put(A2, a1);
      if (mzd_equal(A.m, A2.m)) FAIL("mzd_equal misses the last bit %d x %d", r, c);
      Mat Other = make(r, c + 1, win);
      if (mzd_equal(A.m, Other.m)) FAIL("mzd_equal of two shapes");
      release(Z), release(A), release(A2), release(Other);
      ++n_pred;
    }
    for (unsigned value = 0; value < 2; ++value) {  // mzd_set_ui
      Mat A = make(r, c, win, &a);
      Dense s((size_t)r * w, 0);
      for (int i = 0; value && i < std::min(r, c); ++i) setbit(&s[(size_t)i * w], i, 1);
      mzd_set_ui(A.m, value);
      expect(A, s, "mzd_set_ui", r, c, (int)value);
      release(A);
      ++n_ui;
    }
    {  // mzd_make_table: T[L[v]] = XOR of the rows r0 + j with bit j of v set, from word c0 / 64 on
      const int k = std::min(r, 4), row0 = (int)(rng() % (r - k + 1)), col0 = (int)(rng() % c), w0 = col0 / 64;
      Mat A = make(r, c, win, &a), T = make(1 << k, c, win);
      const Dense t0 = dense(T.m);
      std::vector<rci_t> L(1 << k, -1);
      mzd_make_table(A.m, row0, col0, k, T.m, L.data());
      const Dense t = dense(T.m);
      std::vector<char> seen(1 << k, 0);
      for (int v = 0; v < (1 << k); ++v) {
        if (L[v] < 0 || L[v] >= (1 << k) || seen[L[v]]++) FAIL("mzd_make_table %d x %d: L", r, c);
        for (int q = 0; q < w; ++q) {
          u64 x = 0;
          for (int j = 0; j < k; ++j)
            if ((v >> j) & 1) x ^= a[(size_t)(row0 + j) * w + q];
          const u64 have = t[(size_t)L[v] * w + q];  // words left of c0 stay as they were
          if (q >= w0 ? have != x : have != t0[(size_t)L[v] * w + q]) FAIL("mzd_make_table %d x %d k %d v %d word %d", r, c, k, v, q);
        }
      }
      outside(T, "mzd_make_table", r, c);
      unchanged(A, "mzd_make_table", r, c);
      release(A), release(T);
      ++n_tab;
    }
    for (int v = 0; v < 4; ++v) {  // mzd_apply_p_*: whole permutations and windows of permutations
      const int len_full = v < 2 ? r : c;
      mzp_t *P = mzp_init(len_full);
      for (int i = 0; i < len_full; ++i)
        if (P->values[i] != i) FAIL("mzp_init");
      for (int i = 0; i < len_full; ++i) P->values[i] = i + (int)(rng() % (len_full - i));
      const int begin = len_full / 3;
      mzp_t *W = mzp_init_window(P, 0, len_full - begin), *C = mzp_copy(nullptr, P);
      if (W->length != len_full - begin || W->values != P->values || memcmp(C->values, P->values, sizeof(rci_t) * len_full)) FAIL("mzp window / copy");
      for (const mzp_t *p : {(const mzp_t *)P, (const mzp_t *)W}) {
        Mat A = make(r, c, win, &a);
        Dense s = a;
        oracle_apply_p(s.data(), w, r, c, p->values, p->length, v >> 1, v & 1);
        if (v == 0) mzd_apply_p_left(A.m, p);
        else if (v == 1) mzd_apply_p_left_trans(A.m, p);
        else if (v == 2) mzd_apply_p_right(A.m, p);
        else mzd_apply_p_right_trans(A.m, p);
        expect(A, s, "mzd_apply_p", r, c, v);
        release(A);
        ++n_perm;
      }
      mzp_set_ui(C, 1);
      for (int i = 0; i < len_full; ++i)
        if (C->values[i] != i) FAIL("mzp_set_ui");
      mzp_free_window(W);
      mzp_free(C);
      mzp_free(P);
    }
    {  // gf2_mzd_save and its loader
      const std::string path = dir + "/m.gf2m";
      Mat A = make(r, c, win, &a);
      if (gf2_mzd_save(path.c_str(), A.m) != 0) FAIL("gf2_mzd_save");
      mzd_t *B = gf2_mzd_load(path.c_str());
      if (!B || B->nrows != r || B->ncols != c || dense(B) != a) FAIL("gf2_mzd_load %d x %d", r, c);
      for (int i = 0; i < r; ++i)
        if (B->rows[i][w - 1] & ~lastmask(c)) FAIL("gf2_mzd_load: excess bits");
      mzd_free(B);
      unchanged(A, "gf2_mzd_save", r, c);
      release(A);
      ++n_file;
    }
  }
  for (int nn : DIMS) for (int win = 0; win < 2; ++win) for (int rep = 0; rep < 6; ++rep) for (int given = 0; given < 2; ++given) {  // mzd_invert_naive
    const int w = wordsof(nn);
    Dense a = random_dense(nn, nn);
    if (rep & 1) {  // a product of unit triangular matrices: invertible
      Dense l = random_dense(nn, nn), u = random_dense(nn, nn);
      for (int i = 0; i < nn; ++i)
        for (int j = 0; j < nn; ++j) setbit(&l[(size_t)i * w], j, j < i ? getbit(&l[(size_t)i * w], j) : j == i), setbit(&u[(size_t)i * w], j, j > i ? getbit(&u[(size_t)i * w], j) : j == i);
      oracle_mul_naive(a.data(), w, l.data(), w, u.data(), w, nn, nn, nn);
    }
    Dense inv((size_t)nn * w, 0);
    const bool singular = oracle_inverse(inv.data(), w, a.data(), w, nn) != 0;
    if ((rep & 1) && singular) FAIL("invert driver");
    Mat A = make(nn, nn, win, &a), I = make(nn, nn, win);
    mzd_set_ui(I.m, 1);
    seal(I);
    Mat Out = make(nn, nn, win);
    mzd_t *got = mzd_invert_naive(given ? Out.m : nullptr, A.m, rep & 2 ? I.m : nullptr);
    if ((got == nullptr) != singular) FAIL("mzd_invert_naive %d: singular", nn);
    if (got && given) expect(Out, inv, "mzd_invert_naive", nn, nn);
    else if (got && dense(got) != inv) FAIL("mzd_invert_naive fresh %d", nn);
    if (!got && given) unchanged(Out, "mzd_invert_naive of a singular matrix", nn, nn);
    if (got && !given) mzd_free(got);
    unchanged(A, "mzd_invert_naive", nn, nn), unchanged(I, "mzd_invert_naive", nn, nn);
    release(A), release(I), release(Out);
    ++n_inv;
  }
  report("mzd_init_window", n_win);
  report("mzd_copy", n_copy);
  report("mzd_transpose", n_tr);
  report("mzd_add / mzd_sub", n_add);
  report("mzd_concat", n_cat);
  report("mzd_stack", n_stack);
  report("mzd_submatrix", n_sub);
  report("mzd_row_swap / mzd_copy_row", n_rows);
  report("mzd_col_swap", n_cols);
  report("mzd_row_clear_offset", n_clear);
  report("mzd_is_zero / mzd_equal", n_pred);
  report("mzd_set_ui", n_ui);
  report("mzd_make_table", n_tab);
  report("mzd_invert_naive", n_inv);
  report("mzd_apply_p / mzp", n_perm);
  report("gf2_mzd_save / gf2_mzd_load", n_file);
}

// a block of the pinning size with a device present and hipHostMalloc failing: the pool falls back to a plain allocation
static void run_pinned_fallback() {
  g_stub_devices = 1;
  const int before = g_stub_pin_requests;
  mzd_t *M = mzd_init(1024, 8192);  // 1 MiB: the pinning threshold
  if (g_stub_pin_requests != before + 1) FAIL("pinned pool: hipHostMalloc was not asked");
  if (gf2_mzd_block_is_pinned(M)) FAIL("pinned pool: a failed pin counts as pinned");
  for (int i = 0; i < 1024; ++i)
    for (int j = 0; j < M->width; ++j)
      if (M->rows[i][j]) FAIL("pinned pool: the fallback block is not cleared");
  M->rows[1023][M->width - 1] = ~0ull;  // the last word of the block is ours
  mzd_free(M);
  if (gf2_pinned_alloc(4096) != nullptr) FAIL("pinned pool: gf2_pinned_alloc of a failed pin");
  g_stub_devices = 0;
  report("pinned pool fallback", 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the aliasing predicates of dev_args.h, which every device-resident entry relies on, against enumerated sets of bits and bytes.  The
// addresses are numbers: nothing is read through them.
// ---------------------------------------------------------------------------------------------------------------------------------
static void run_arg_rules() {
  long n = 0;
  const long long BASE = 1ll << 20;  // a bit address for the rectangles, a byte address for the ranges
  static unsigned char in_x[4096];
  const int COLS[] = {1, 63, 64, 65, 128, 130};
  // rectangles of bits: X at BASE + 37 (its first bit lies inside a word), Y at every distance at which the two can meet, and beyond
  for (int ldx = 1; ldx <= 3; ++ldx) for (int ldy = 1; ldy <= 3; ++ldy) for (int xr = 1; xr <= 3; ++xr) for (int xc : COLS) {
    if (xc > 64 * ldx) continue;
    const int reach_x = (xr - 1) * 64 * ldx + xc;  // bits from the first to one past the last
    memset(in_x, 0, sizeof in_x);
    for (int i = 0; i < xr; ++i)
      for (int j = 0; j < xc; ++j) in_x[1024 + i * 64 * ldx + j] = 1;
    for (int yr = 1; yr <= 3; ++yr) for (int yc : COLS) {
      if (yc > 64 * ldy) continue;
      const int reach_y = (yr - 1) * 64 * ldy + yc;
      if (reach_x + 70 > 1024 || reach_y + 70 > 1024) FAIL("arg rules driver: the window is too small");
      // with one stride every distance; with two, where the answer may be anything but "no" is required, every 5th
      for (int d = -(reach_y + 69); d <= reach_x + 69; d += ldx == ldy ? 1 : 5) {
        bool share = false;
        for (int i = 0; i < yr && !share; ++i)
          for (int j = 0; j < yc && !share; ++j) share = in_x[1024 + d + i * 64 * ldy + j];
        const bool got = gf2_bit_rects_share((__int128)BASE + 37, ldx, xr, xc, (__int128)BASE + 37 + d, ldy, yr, yc);
        if (ldx == ldy ? got != share : share && !got)
          FAIL("gf2_bit_rects_share: ld %d / %d, %d x %d and %d x %d at distance %d: %d, the bits say %d", ldx, ldy, xr, xc, yr, yc, d, got, share);
        ++n;
      }
    }
  }
  // byte ranges: flat against flat
  auto ptr = [&](long long byte) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(BASE + byte)); };
  for (int a = 0; a < 24; ++a) for (int la : {0, 1, 2, 5, 12}) for (int b = 0; b < 24; ++b) for (int lb : {0, 1, 2, 5, 12}) {
    bool share = false;
    for (int x = a; x < a + la; ++x) share |= x >= b && x < b + lb;
    if (gf2_ranges_meet(ptr(a), la, ptr(b), lb) != share) FAIL("gf2_ranges_meet: [%d, +%d) and [%d, +%d)", a, la, b, lb);
    ++n;
  }
  // a matrix's range: every byte from the first of its words to the last, the padding of the rows in between included
  typedef std::vector<char> Bytes;  // of a window of 160 bytes at BASE
  auto bytes_of = [&](const gf2_dmat &M) {
    Bytes s(160, 0);
    int lo = 160, hi = 0;
    for (int i = 0; i < M.nrows; ++i)
      for (int w = 0; w < wordsof(M.ncols); ++w) {
        const int at = (int)(reinterpret_cast<uintptr_t>(M.data) - BASE) + 8 * (i * (int)M.ld + w);
        lo = std::min(lo, at), hi = std::max(hi, at + 8);
      }
    for (int x = lo; x < hi; ++x) s[x] = 1;
    return s;
  };
  std::vector<gf2_dmat> mats;
  for (int at : {0, 8, 24}) for (int r = 0; r <= 3; ++r) for (int c : {0, 1, 64, 65}) for (int pad = 0; pad < 2; ++pad) {
    gf2_dmat M{};
    M.data = reinterpret_cast<uint64_t *>(static_cast<uintptr_t>(BASE + 40 + at));
    M.nrows = r, M.ncols = c, M.ld = std::max(1, wordsof(c)) + pad;
    mats.push_back(M);
  }
  for (const gf2_dmat &M : mats) {
    const Bytes m = bytes_of(M);
    const int m0 = (int)(reinterpret_cast<uintptr_t>(M.data) - BASE);
    for (int a = 0; a < 150; ++a) for (int la : {0, 1, 4, 9}) {
      bool share = false;
      for (int x = a; x < a + la; ++x) share |= m[x] != 0;
      if (gf2_range_meets_mat(ptr(a), la, &M) != share)
        FAIL("gf2_range_meets_mat: [%d, +%d) and a %d x %d matrix at %d, ld %d", a, la, M.nrows, M.ncols, m0, (int)M.ld);
      ++n;
    }
    for (const gf2_dmat &Y : mats) {
      const Bytes y = bytes_of(Y);
      bool share = false;
      for (int x = 0; x < 160; ++x) share |= m[x] && y[x];
      if (gf2_mat_ranges_meet(&M, &Y) != share)
        FAIL("gf2_mat_ranges_meet: %d x %d at %d, ld %d, and %d x %d at %d, ld %d", M.nrows, M.ncols, m0, (int)M.ld, Y.nrows, Y.ncols,
             (int)(reinterpret_cast<uintptr_t>(Y.data) - BASE), (int)Y.ld);
      ++n;
    }
  }
  report("dev_args.h overlap predicates", n);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("usage: host_san <scratch directory>\n");
    return 2;
  }
  run_arg_rules();
  run_echelonize();
  run_ple();
  run_trsm();
  run_nullspace();
  run_mul();
  run_containers(argv[1]);
  run_pinned_fallback();
  printf("all ok\n");
  return 0;
}
