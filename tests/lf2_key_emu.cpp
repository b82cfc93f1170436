// lf2_key_emu.cpp -- the word-level helpers of the LF2 kernels (lf2_window / lf2_key, lf2_class_start, lf2_find_position of
// m4ri-rust_amd/csrc/lf2/gf2_lf2.hip, cut out of the shipped file by tests/test_lf2_key_cpu.py) on the CPU under the host compiler's
// address and undefined-behaviour sanitizers.
//   the key: every row lives in a heap block of its own that ENDS with the last word of the row; a second run gives the function a
//   block that holds ONLY the words with a bit of the window (none for b == 0).  A read of any other word is a sanitizer report.
//   the class start: sorted keys in a heap block that ends with position s0, against a walk back.
//   the position of an output: sums with empty positions, with one giant position and with 64-bit totals, against a linear search.
#include "kernel_emu.h"

namespace {
#include KERNEL_BODY
}

static u32 key_by_bits(const u64 *row, int c0, int b) {
  u32 v = 0;
  for (int j = 0; j < b; ++j) v |= (u32)((row[(c0 + j) >> 6] >> ((c0 + j) & 63)) & 1) << j;
  return v;
}

static long check_keys() {
  const int widths[] = {1, 63, 64, 65, 128, 130};
  std::mt19937_64 rng(2026);
  long cases = 0;
  for (int ncols : widths) {
    const int nw = (ncols + 63) >> 6;
    for (int rep = 0; rep < 3; ++rep) {
      u64 *row = new u64[nw];  // the block ends with the row's last word
      for (int k = 0; k < nw; ++k) row[k] = rep == 0 ? rng() : rep == 1 ? ~0ull : (0xAAAAAAAAAAAAAAAAull >> (k & 1));
      for (int c0 = 0; c0 <= ncols; ++c0)
        for (int b = 0; b <= 30 && c0 + b <= ncols; ++b) {
          const u32 want = key_by_bits(row, c0, b);
          const Lf2Window w = lf2_window(c0, b);
          if (lf2_key(row, w) != want) {
            printf("ncols %d c0 %d b %d: key %u, by bits %u\n", ncols, c0, b, lf2_key(row, w), want);
            return -1;
          }
          // only the words of the window: [first, last], none for b == 0
          const int first = c0 >> 6, last = b ? (c0 + b - 1) >> 6 : first - 1, held = last - first + 1;
          if (held < 0 || held > 2) {
            printf("ncols %d c0 %d b %d: %d words\n", ncols, c0, b, held);
            return -1;
          }
          u64 *part = new u64[held];
          for (int k = 0; k < held; ++k) part[k] = row[first + k];
          const u64 *shifted = reinterpret_cast<const u64 *>(reinterpret_cast<uintptr_t>(part) - 8 * (uintptr_t)first);
          if (lf2_key(shifted, w) != want) {
            printf("ncols %d c0 %d b %d: key of the window's words alone differs\n", ncols, c0, b);
            return -1;
          }
          delete[] part;
          ++cases;
        }
      delete[] row;
    }
  }
  return cases;
}

// class sizes of every shape in front of s0: the start is found, and nothing behind s0 is read
static long check_class_starts() {
  std::mt19937_64 rng(7);
  long cases = 0;
  const int sizes[] = {1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1000, 4097};
  for (int before : {0, 1, 2, 5, 100})      // positions of smaller keys in front of the class
    for (int size : sizes)
      for (int at = 0; at < size; at += (size > 70 ? 61 : 1)) {   // s0 = the at-th member of the class
        const long long s0 = before + at;
        int *k = new int[s0 + 1];  // the block ends with position s0
        for (int i = 0; i < before; ++i) k[i] = (int)(rng() % 3) + (i ? k[i - 1] : 0);
        const int v = (before ? k[before - 1] : 0) + 1 + (int)(rng() % 2);
        for (long long i = before; i <= s0; ++i) k[i] = v;
        const long long got = lf2_class_start(k, s0);
        if (got != before) {
          printf("class of %d at %d behind %d smaller keys: start %lld\n", size, at, before, got);
          return -1;
        }
        delete[] k;
        ++cases;
      }
  return cases;
}

static long check_positions() {
  std::mt19937_64 rng(11);
  long cases = 0;
  for (int kind = 0; kind < 5; ++kind)
    for (int n : {1, 2, 3, 64, 1000, 1024}) {
      std::vector<long long> r(n), pre(n);
      for (int q = 0; q < n; ++q) {
        switch (kind) {
          case 0: r[q] = (long long)(rng() % 4); break;                          // many empty positions
          case 1: r[q] = q == n / 2 ? 3000000000ll : 0; break;                   // one giant position, the rest empty
          case 2: r[q] = (long long)q + 2000000000ll; break;                     // a class that began long before: 64-bit totals
          case 3: r[q] = q == n - 1 ? 5 : 0; break;                              // only the last position
          default: r[q] = q == 0 ? 7 : (long long)(rng() % 2); break;
        }
      }
      long long total = 0;
      for (int q = 0; q < n; ++q) {
        pre[q] = total;
        total += r[q];
      }
      if (total == 0) continue;
      long long *p = new long long[n];  // a heap block of exactly n sums
      std::copy(pre.begin(), pre.end(), p);
      std::vector<long long> js = {0, total - 1, total / 2, total / 3};
      for (int q = 0; q < n; ++q)
        if (r[q]) {
          js.push_back(pre[q]);
          js.push_back(pre[q] + r[q] - 1);
        }
      for (long long j : js) {
        int want = 0;
        while (!(pre[want] <= j && j < pre[want] + r[want])) ++want;
        const int got = lf2_find_position(p, n, j);
        if (got != want) {
          printf("kind %d n %d output %lld: position %d, by search %d\n", kind, n, j, got, want);
          return -1;
        }
        ++cases;
      }
      delete[] p;
    }
  return cases;
}

int main() {
  const long keys = check_keys();
  if (keys < 0) return 1;
  printf("%ld keys ok\n", keys);
  const long starts = check_class_starts();
  if (starts < 0) return 1;
  printf("%ld class starts ok\n", starts);
  const long positions = check_positions();
  if (positions < 0) return 1;
  printf("%ld positions ok\n", positions);
  return 0;
}
