// join_select_emu.cpp -- the word-level helpers of the weight-filtered join (join_select_first_word, join_select_end_word,
// join_select_is_hit and join_select_pair_weight of m4ri-rust_amd/csrc/join/gf2_join_select.inc, with gf2_word_weight, gf2_lo_hi and
// gf2_load2 of gf2_dev_words.h that they call; cut out of the shipped files by tests/test_join_select_helpers_cpu.py) on the CPU under
// the host compiler's address and undefined-behaviour sanitizers.
//   the words of a range: for every [wc0, wc1) of a row of ncols bits, [first, end) are exactly the words that hold a column of the
//   range, and the weights of those words alone (gf2_word_weight) sum to the bit-by-bit count.
//   the weight of a pair: rows a and p in heap blocks of exactly the row's words (16-byte aligned, so that the 16-byte form may run
//   too), dealt to 1, 2, 8 and 64 lanes, with and without 16-byte accesses: the lanes' sums equal the bit-by-bit count of a ^ p on the
//   range, excess bits of the last word set or not.  A read of a word behind the row is an error of the address sanitizer.
//   the window: for every range and every 0 <= wlo <= whi <= width + 2, the predicate on the helpers' weight equals the predicate on
//   the bit-by-bit count.
#include "kernel_emu.h"

namespace {
#include KERNEL_BODY
}

int main() {
  const int widths[] = {1, 63, 64, 65, 130};
  std::mt19937_64 rng(2027);
  long ranges = 0, windows = 0, pairs = 0;
  for (int ncols : widths) {
    const int nw = (ncols + 63) >> 6;
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<u64> a(nw), p(nw);
      for (int k = 0; k < nw; ++k) {
        a[k] = rep == 1 ? ~0ull : rng();
        p[k] = rep == 1 ? 0ull : rep == 2 ? a[k] ^ (0xAAAAAAAAAAAAAAAAull >> (k & 1)) : rng();  // excess bits of the last word are dirty
      }
      u64 *ha = static_cast<u64 *>(malloc(8 * nw)), *hp = static_cast<u64 *>(malloc(8 * nw));  // malloc: 16-byte aligned, exactly nw words
      std::copy(a.begin(), a.end(), ha);
      std::copy(p.begin(), p.end(), hp);
      if ((reinterpret_cast<uintptr_t>(ha) | reinterpret_cast<uintptr_t>(hp)) & 15) {
        printf("the heap blocks are not 16-byte aligned\n");
        return 1;
      }
      for (int wc0 = 0; wc0 <= ncols; ++wc0)
        for (int wc1 = wc0; wc1 <= ncols; ++wc1) {
          int want = 0;
          for (int c = wc0; c < wc1; ++c) want += (int)(((a[c >> 6] ^ p[c >> 6]) >> (c & 63)) & 1);
          const long long first = join_select_first_word(wc0, wc1), end = join_select_end_word(wc0, wc1);
          if (first < 0 || first > end || end > nw) {
            printf("ncols %d [%d, %d): words [%lld, %lld)\n", ncols, wc0, wc1, first, end);
            return 1;
          }
          int got = 0;
          for (long long k = 0; k < nw; ++k) {
            const bool holds = wc0 < wc1 && 64 * k < wc1 && wc0 < 64 * (k + 1);
            if (holds != (k >= first && k < end)) {
              printf("ncols %d [%d, %d): word %lld is %s the range, the helpers say [%lld, %lld)\n", ncols, wc0, wc1, k, holds ? "in" : "outside",
                     first, end);
              return 1;
            }
            if (holds) got += gf2_word_weight(a[k] ^ p[k], k, wc0, wc1);
          }
          if (got != want) {
            printf("ncols %d [%d, %d): weight %d over the words of the range, by bits %d\n", ncols, wc0, wc1, got, want);
            return 1;
          }
          ++ranges;
          for (int lanes : {1, 2, 8, 64})
            for (int vec = 0; vec < 2; ++vec) {
              if (vec && nw < 2) continue;  // 16-byte accesses need a pair of words (gf2_rows_aligned16)
              int sum = 0;
              for (int sub = 0; sub < lanes; ++sub) sum += join_select_pair_weight(ha, hp, nw, vec, vec, sub, lanes, wc0, wc1);
              if (sum != want) {
                printf("ncols %d [%d, %d) lanes %d vec %d: pair weight %d, by bits %d\n", ncols, wc0, wc1, lanes, vec, sum, want);
                return 1;
              }
              ++pairs;
            }
          const int width = wc1 - wc0;
          for (int wlo = 0; wlo <= width + 2; ++wlo)
            for (int whi = wlo; whi <= width + 2; ++whi) {
              const int hit = join_select_is_hit(got, wlo, whi);
              if (hit != (wlo <= want && want <= whi)) {
                printf("ncols %d [%d, %d) weight %d window [%d, %d]: hit %d\n", ncols, wc0, wc1, want, wlo, whi, hit);
                return 1;
              }
              ++windows;
            }
        }
      free(ha);
      free(hp);
    }
  }
  printf("%ld ranges ok\n%ld pair weights ok\n%ld windows ok\n", ranges, pairs, windows);
  return 0;
}
