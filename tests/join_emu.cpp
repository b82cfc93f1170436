// join_emu.cpp -- the word-level helpers that the join kernels keep for themselves (join_lower_bound and join_upper_bound of
// m4ri-rust_amd/csrc/join/gf2_join.hip, cut out of the shipped file by tests/test_join_helpers_cpu.py) on the CPU under the host
// compiler's address and undefined-behaviour sanitizers.  The position of an output and the weight of a column range are shared
// helpers: dev_words_emu.cpp.
//   the bounds: sorted keys in a heap block of exactly hi ints, handed over shifted so that only [lo, hi) may be read, against a
//   linear walk: the first and the last element, keys that are absent, below all and above all, one giant class.
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

int main() {
  const long bounds = check_bounds();
  if (bounds < 0) return 1;
  printf("%ld bounds ok\n", bounds);
  return 0;
}
