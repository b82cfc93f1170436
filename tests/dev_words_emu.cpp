// dev_words_emu.cpp -- the word-level helpers that the LPN modules share (gf2_key_window / gf2_row_key, gf2_word_mask, gf2_word_weight
// and gf2_find_position of m4ri-rust_amd/csrc/gf2_dev_words.h, cut out of the shipped file by tests/test_dev_words_cpu.py) on the CPU
// under the host compiler's address and undefined-behaviour sanitizers: the cases that bkw_key_emu.cpp, lf2_key_emu.cpp, join_emu.cpp,
// sums_emu.cpp and near_emu.cpp ran on the modules' own copies.
//   the key: every row lives in a heap block of its own that ENDS with the last word of the row; a second run gives the function a
//   block that holds ONLY the words with a bit of the window (none for b == 0).  A read of any other word is a sanitizer report.
//   the mask and the weight of a column range: every [wc0, wc1) of a row of ncols bits, word by word (each in a heap block of its own),
//   against the bits written out; a word outside the range has no bit and counts nothing, and the weight is the popcount under the mask.
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
          const Gf2KeyWindow w = gf2_key_window(c0, b);
          if (gf2_row_key(row, w) != want) {
            printf("ncols %d c0 %d b %d: key %u, by bits %u\n", ncols, c0, b, gf2_row_key(row, w), want);
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
          if (gf2_row_key(shifted, w) != want) {
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
            u64 bits = 0;  // the columns of the range in word k, one by one
            for (int c = wc0; c < wc1; ++c)
              if ((c >> 6) == k) bits |= 1ull << (c & 63);
            u64 *word = new u64[1];  // a word of the range in a block of its own
            word[0] = row[k];
            const int w = gf2_word_weight(word[0], k, wc0, wc1);
            const u64 m = gf2_word_mask(k, wc0, wc1);
            delete[] word;
            if (!holds && (w != 0 || m != 0)) {
              printf("ncols %d [%d, %d): word %d is outside the range, counts %d and has the mask %llx\n", ncols, wc0, wc1, k, w,
                     (unsigned long long)m);
              return -1;
            }
            if (m != bits || w != __popcll(row[k] & m)) {
              printf("ncols %d [%d, %d): the mask or the weight of word %d\n", ncols, wc0, wc1, k);
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
          case 2: r[q] = (long long)q + 2000000000ll; break;                     // a giant class: 64-bit totals
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
        const int got = gf2_find_position(p, n, j);
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
  const long weights = check_weights();
  if (weights < 0) return 1;
  printf("%ld weights ok\n", weights);
  const long positions = check_positions();
  if (positions < 0) return 1;
  printf("%ld positions ok\n", positions);
  return 0;
}
