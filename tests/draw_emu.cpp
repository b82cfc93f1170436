// draw_emu.cpp -- the SHIPPED generator and per-word rules of the device draws (m4ri-rust_amd/csrc/draw/philox.h, included as it is:
// the kernels of gf2_draw.hip call these functions and nothing else to make a value) on the CPU under the host compiler's address and
// undefined-behaviour sanitizers.  It prints what the functions give for a fixed list of inputs, one line per call;
// tests/test_draw_philox_cpu.py holds every line to the yardstick of tests/draw_ref.py.
//   K c0 c1 c2 c3 k0 k1 -> x0 x1 x2 x3      philox4x32_10 (the published known answers are among them)
//   B seed widx thr -> word                  draw_bernoulli_word
//   I seed p n -> even odd                   draw_index_pair
//   S seed at round n -> v                   draw_subset_candidate
//   P seed i -> key                          draw_perm_key
//   C thr -> calls                           16 - draw_bernoulli_first_call
// Every number is hexadecimal.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "philox.h"

typedef unsigned long long ull;

int main() {
  const uint32_t known[][6] = {{0, 0, 0, 0, 0, 0},
                               {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                               {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u},
                               {1, 2, 3, 4, 5, 6}};
  for (const auto &c : known) {
    const Philox4 x = philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5]);
    printf("K %08x %08x %08x %08x %08x %08x -> %08x %08x %08x %08x\n", c[0], c[1], c[2], c[3], c[4], c[5], x.x0, x.x1, x.x2, x.x3);
  }
  const uint64_t seeds[] = {0, 9, 0xDEADBEEFCAFEF00Dull};
  const uint64_t places[] = {0, 1, 2, 63, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0x8000000000000005ull, ~0ull};
  const uint32_t thrs[] = {0, 1, 2, 0x20000000u, 0x40000000u, 0x80000000u, 0x12345679u, 0x12345678u, 0xFFFFFFFFu, 0xFFFF0000u};
  const uint32_t ns[] = {1, 2, 3, 1000, 0x7FFFFFFFu};
  for (uint64_t seed : seeds)
    for (uint64_t at : places) {
      for (uint32_t thr : thrs) printf("B %llx %llx %x -> %llx\n", (ull)seed, (ull)at, thr, (ull)draw_bernoulli_word(seed, at, thr));
      for (uint32_t n : ns) {
        uint32_t even, odd;
        draw_index_pair(seed, at, n, &even, &odd);
        printf("I %llx %llx %x -> %x %x\n", (ull)seed, (ull)at, n, even, odd);
        for (uint32_t round : {0u, 1u, 63u}) printf("S %llx %llx %x %x -> %x\n", (ull)seed, (ull)at, round, n, draw_subset_candidate(seed, at, round, n));
      }
      printf("P %llx %x -> %x\n", (ull)seed, (uint32_t)at, draw_perm_key(seed, (uint32_t)at));
    }
  for (uint32_t thr : thrs) printf("C %x -> %x\n", thr, 16 - draw_bernoulli_first_call(thr));
  return 0;
}
