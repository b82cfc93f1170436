// unique_emu.cpp -- the rekey kernel and the row compare of the row sort (gf2_unique_rekey_kernel and unique_rows_differ of
// m4ri-rust_amd/csrc/unique/gf2_unique.hip, with gf2_key_window, gf2_row_key and gf2_word_mask of gf2_dev_words.h, which they use; cut
// out of the shipped files by tests/test_unique_kernels_cpu.py; unique_plan.h is plain host arithmetic and is included as it is) on the
// CPU, thread by thread, under the host compiler's address and undefined-behaviour sanitizers.
//   the keys: for every range [c0, c1) of a row of ncols bits and every window of it (unique_plan.h cuts them), the kernel runs on ONE
//   row that lives in a heap block of ONLY the words that hold a bit of that window, as the first window (the identity order) and as a
//   later one (the row comes from the pair).  The key must equal the window's bits written out one by one, and the windows of a range
//   must cover it exactly once, least significant first.  Then a launch of two workgroups over a permuted order of 300 rows.
//   the compare: two rows in heap blocks of ONLY the words of the range.  Equal on the range with every bit outside it flipped:
//   equal.  One column of the range flipped, for every column: different, and the blocks END with the word of that column -- the
//   compare may not read on behind the first difference.
// A read of any other word is a report of the address sanitizer.
#include "kernel_emu.h"
#include "unique_plan.h"  // m4ri-rust_amd/csrc/unique, as shipped

namespace {
#include KERNEL_BODY
}

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return -1;           \
  } while (0)

static int bit_of(const std::vector<u64> &row, int c) { return (int)((row[c >> 6] >> (c & 63)) & 1); }

// a heap block of the words [w0, w1) of `row` alone, addressed like the row
struct Part {
  u64 *block;
  const u64 *row;
  Part(const std::vector<u64> &full, long long w0, long long w1) {
    block = new u64[w1 - w0];
    for (long long k = w0; k < w1; ++k) block[k - w0] = full[k];
    row = reinterpret_cast<const u64 *>(reinterpret_cast<uintptr_t>(block) - 8 * (uintptr_t)w0);
  }
  ~Part() { delete[] block; }
};

static void launch_rekey(const u64 *P, long long ld, int wc0, int bits, long long n, int first, int2 *pairs) {
  hipLaunchKernelGGL(gf2_unique_rekey_kernel, dim3((unsigned)((n + kUniqueThreads - 1) / kUniqueThreads)), dim3(kUniqueThreads), 0, nullptr, P,
                     ld, wc0, bits, n, first, pairs);
}

static long check_keys(const int *widths, int nwidths) {
  std::mt19937_64 rng(2031);
  long cases = 0;
  for (int t = 0; t < nwidths; ++t) {
    const int ncols = widths[t], nw = (ncols + 63) >> 6;
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<u64> row(nw);
      for (int k = 0; k < nw; ++k) row[k] = rep == 0 ? rng() : rep == 1 ? ~0ull : (0xAAAAAAAAAAAAAAAAull >> (k & 1));  // excess bits are dirty
      for (int c0 = 0; c0 <= ncols; ++c0)
        for (int c1 = c0; c1 <= ncols; ++c1) {
          const UniquePlan plan = unique_plan(1, ncols, c0, c1);
          if (plan.windows != (c1 - c0 + kUniqueWindowBits - 1) / kUniqueWindowBits) FAIL("ncols %d [%d, %d): %d windows", ncols, c0, c1, plan.windows);
          int at = c0;  // the windows cover the range once, from c0 upward
          for (int win = 0; win < plan.windows; ++win) {
            const int wc0 = unique_window_c0(c0, win), bits = unique_window_bits(c0, c1, win);
            if (wc0 != at || bits < 1 || bits > kUniqueWindowBits || (win < plan.windows - 1 && bits != kUniqueWindowBits))
              FAIL("ncols %d [%d, %d): window %d is [%d, %d + %d)", ncols, c0, c1, win, wc0, wc0, bits);
            at += bits;
            u32 want = 0;
            for (int j = 0; j < bits; ++j) want |= (u32)bit_of(row, wc0 + j) << j;
            const Part part(row, unique_first_word(wc0, wc0 + bits), unique_end_word(wc0, wc0 + bits));
            for (int first = 0; first < 2; ++first) {
              int2 *pair = new int2[1];
              pair[0] = make_int2(0x5EAD, first ? 77 : 0);  // first: the pair is not read
              launch_rekey(part.row, 1000, wc0, bits, 1, first, pair);
              const bool ok = (u32)pair[0].x == want && pair[0].y == 0;
              delete[] pair;
              if (!ok) FAIL("ncols %d [%d, %d) window %d first %d: the key or the row", ncols, c0, c1, win, first);
            }
          }
          if (at != c1) FAIL("ncols %d [%d, %d): the windows end at %d", ncols, c0, c1, at);
          ++cases;
        }
    }
  }
  // two workgroups, a permuted order: pairs[i] = (key of row r, r) for the r that the pair held
  const int n = 300, ncols = 130, ld = 5;
  std::vector<u64> P((size_t)n * ld);
  for (auto &x : P) x = rng();
  std::vector<int> perm(n);
  for (int i = 0; i < n; ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  for (int first = 0; first < 2; ++first) {
    int2 *pairs = new int2[n];
    for (int i = 0; i < n; ++i) pairs[i] = make_int2(-1, perm[i]);
    launch_rekey(P.data(), ld, 57, 24, n, first, pairs);
    for (int i = 0; i < n; ++i) {
      const int r = first ? i : perm[i];
      u32 want = 0;
      for (int j = 0; j < 24; ++j) want |= (u32)((P[(size_t)r * ld + ((57 + j) >> 6)] >> ((57 + j) & 63)) & 1) << j;
      if (pairs[i].y != r || (u32)pairs[i].x != want) FAIL("the launch of two workgroups: pair %d", i);
    }
    delete[] pairs;
    ++cases;
  }
  return cases;
}

static long check_compares(const int *widths, int nwidths) {
  std::mt19937_64 rng(2032);
  long cases = 0;
  for (int t = 0; t < nwidths; ++t) {
    const int ncols = widths[t], nw = (ncols + 63) >> 6;
    std::vector<u64> a(nw);
    for (int k = 0; k < nw; ++k) a[k] = rng();
    for (int c0 = 0; c0 <= ncols; ++c0)
      for (int c1 = c0; c1 <= ncols; ++c1) {
        const long long w0 = unique_first_word(c0, c1), w1 = unique_end_word(c0, c1);
        if (c0 < c1 && (w0 != (c0 >> 6) || w1 != ((c1 - 1) >> 6) + 1)) FAIL("ncols %d [%d, %d): words [%lld, %lld)", ncols, c0, c1, w0, w1);
        if (c0 == c1 && w0 != w1) FAIL("ncols %d: the empty range [%d, %d) holds a word", ncols, c0, c1);
        std::vector<u64> b(nw);
        for (int k = 0; k < nw; ++k) b[k] = ~a[k];  // every bit outside the range differs, the excess bits too ...
        for (int c = c0; c < c1; ++c) b[c >> 6] ^= 1ull << (c & 63);  // ... and inside it none
        {
          const Part pa(a, w0, w1), pb(b, w0, w1);
          if (unique_rows_differ(pa.row, pb.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): rows that are equal on the range differ", ncols, c0, c1);
          if (unique_rows_differ(pa.row, pa.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): a row differs from itself", ncols, c0, c1);
        }
        ++cases;
        for (int c = c0; c < c1; ++c) {  // one column flipped: the blocks end with its word
          b[c >> 6] ^= 1ull << (c & 63);
          const Part pa(a, w0, (c >> 6) + 1), pb(b, w0, (c >> 6) + 1);
          if (!unique_rows_differ(pa.row, pb.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): a difference in column %d is not seen", ncols, c0, c1, c);
          b[c >> 6] ^= 1ull << (c & 63);
          ++cases;
        }
      }
  }
  return cases;
}

int main() {
  const int widths[] = {1, 63, 64, 65, 130};
  const long keys = check_keys(widths, 5);
  if (keys < 0) return 1;
  printf("%ld keys ok\n", keys);
  const long compares = check_compares(widths, 5);
  if (compares < 0) return 1;
  printf("%ld compares ok\n", compares);
  return 0;
}
