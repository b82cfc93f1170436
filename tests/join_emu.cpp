// join_emu.cpp -- the word-level helpers of the join kernels (join_lower_bound, join_upper_bound, join_find_position and
// join_word_weight of m4ri-rust_amd/csrc/join/gf2_join.hip, cut out of the shipped file by tests/test_join_helpers_cpu.py) on the CPU
// under the host compiler's address and undefined-behaviour sanitizers.
//   the bounds: sorted keys in a heap block of exactly hi ints, handed over shifted so that only [lo, hi) may be read, against a
//   linear walk: the first and the last element, keys that are absent, below all and above all, one giant class.
//   the position of an output: sums with empty positions, with one giant position and with 64-bit totals, against a linear search.
//   the weight of a column range: every [wc0, wc1) of a row of ncols bits, summed over the words that hold a bit of the range (each in
//   a heap block of its own), against a bit-by-bit count; words outside the range must count nothing.
#include "kernel_emu.h"

namespace {
#include KERNEL_BODY
}

// keys[lo .. hi) in a block that holds nothing else; the pointer is shifted so that index lo is the block's first element
struct Window {
  int *block;
  const int *keys;
  Window(const std::vector<int> &all, long long lo, long long hi) {
    block = new int[hi - lo];
    for (long long i = lo; i < hi; ++i) block[i - lo] = all[i];
    keys = reinterpret_cast<const int *>(reinterpret_cast<uintptr_t>(block) - 4 * (uintptr_t)lo);
  }
  ~Window() { delete[] block; }
};

static long check_bounds_on(const std::vector<int> &all, const std::vector<int> &probes) {
  const long long n = (long long)all.size();
  long cases = 0;
  const long long cuts[][2] = {{0, n}, {0, 0}, {n, n}, {n / 3, n}, {0, n / 2}, {n / 4, (3 * n) / 4}, {n > 0 ? n - 1 : 0, n}, {0, n > 0 ? 1 : 0}};
  for (const auto &cut : cuts) {
    const long long lo = cut[0], hi = cut[1];
    Window w(all, lo, hi);
    for (int v : probes) {
      long long lb = lo, ub = lo;
      while (lb < hi && all[lb] < v) ++lb;
      while (ub < hi && all[ub] <= v) ++ub;
      const long long got_l = join_lower_bound(w.keys, lo, hi, v), got_u = join_upper_bound(w.keys, lo, hi, v);
      if (got_l != lb || got_u != ub || join_upper_bound(w.keys, got_l, hi, v) != ub) {
        printf("n %lld [%lld, %lld) key %d: bounds %lld %lld, by walk %lld %lld\n", n, lo, hi, v, got_l, got_u, lb, ub);
        return -1;
      }
      ++cases;
    }
  }
  return cases;
}

static long check_bounds() {
  std::mt19937_64 rng(13);
  long cases = 0;
  for (int kind = 0; kind < 5; ++kind)
    for (int n : {0, 1, 2, 3, 64, 1000, 4097}) {
      std::vector<int> all(n);
      int k = 5;
      for (int i = 0; i < n; ++i) {
        switch (kind) {
          case 0: k += (int)(rng() % 3); break;                          // small classes, some keys absent
          case 1: k = 77; break;                                         // one giant class
          case 2: k += 2; break;                                         // all distinct, every odd key absent
          case 3: k = i < n / 2 ? 9 : 0x3FFFFFFF; break;                 // two classes, the largest key there is
          default: k += (i % 97 == 0) ? 1000 : 0; break;                 // long classes
        }
        all[i] = k;
      }
      std::vector<int> probes = {0, 1, 4, 5, 6, 76, 77, 78, 0x3FFFFFFF, 0x3FFFFFFE};
      if (n) {
        probes.insert(probes.end(), {all[0], all[0] - 1, all[0] + 1, all[n - 1], all[n - 1] - 1, all[n - 1] + 1, all[n / 2], all[n / 2] + 1});
        for (int i = 0; i < 20; ++i) probes.push_back(all[rng() % n] + (int)(rng() % 2));
      }
      const long c = check_bounds_on(all, probes);
      if (c < 0) return -1;
      cases += c;
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
          case 2: r[q] = (long long)q + 2000000000ll; break;                     // a giant class of B: 64-bit totals
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
        const int got = join_find_position(p, n, j);
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

static long check_weights() {
  const int widths[] = {1, 63, 64, 65, 130};
  std::mt19937_64 rng(2026);
  long cases = 0;
  for (int ncols : widths) {
    const int nw = (ncols + 63) >> 6;
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<u64> row(nw);
      for (int k = 0; k < nw; ++k) row[k] = rep == 0 ? rng() : rep == 1 ? ~0ull : (0xAAAAAAAAAAAAAAAAull >> (k & 1));
      for (int wc0 = 0; wc0 <= ncols; ++wc0)
        for (int wc1 = wc0; wc1 <= ncols; ++wc1) {
          int want = 0;
          for (int c = wc0; c < wc1; ++c) want += (int)((row[c >> 6] >> (c & 63)) & 1);
          int got = 0;
          for (int k = 0; k < nw; ++k) {
            const bool holds = wc0 < wc1 && 64 * k < wc1 && wc0 < 64 * (k + 1);
            u64 *word = new u64[1];  // a word of the range in a block of its own
            word[0] = row[k];
            const int w = join_word_weight(word[0], k, wc0, wc1);
            delete[] word;
            if (!holds && w != 0) {
              printf("ncols %d [%d, %d): word %d is outside the range and counts %d\n", ncols, wc0, wc1, k, w);
              return -1;
            }
            got += w;
          }
          if (got != want) {
            printf("ncols %d [%d, %d): weight %d, by bits %d\n", ncols, wc0, wc1, got, want);
            return -1;
          }
          ++cases;
        }
    }
  }
  return cases;
}

int main() {
  const long bounds = check_bounds();
  if (bounds < 0) return 1;
  printf("%ld bounds ok\n", bounds);
  const long positions = check_positions();
  if (positions < 0) return 1;
  printf("%ld positions ok\n", positions);
  const long weights = check_weights();
  if (weights < 0) return 1;
  printf("%ld weights ok\n", weights);
  return 0;
}
