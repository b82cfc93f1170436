// lf2_key_emu.cpp -- the word-level helper that the LF2 kernels keep for themselves (lf2_class_start of
// m4ri-rust_amd/csrc/lf2/gf2_lf2.hip, cut out of the shipped file by tests/test_lf2_key_cpu.py) on the CPU under the host compiler's
// address and undefined-behaviour sanitizers.  The key reader and the position of an output are shared helpers: dev_words_emu.cpp.
//   the class start: sorted keys in a heap block that ends with position s0, against a walk back.
#include "kernel_emu.h"

namespace {
#include KERNEL_BODY
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

int main() {
  const long starts = check_class_starts();
  if (starts < 0) return 1;
  printf("%ld class starts ok\n", starts);
  return 0;
}
