// bkw_key_emu.cpp -- the key reader of the LF1 kernels (lf1_window / lf1_key of m4ri-rust_amd/csrc/bkw/gf2_bkw.hip, cut out of the
// shipped file by tests/test_bkw_key_cpu.py) on the CPU under the host compiler's address and undefined-behaviour sanitizers.
// Every row lives in a heap block of its own that ENDS with the last word of the row; a second run gives the function a block that
// holds ONLY the words with a bit of the window (none for b == 0).  A read of any other word is a sanitizer report.
#include "kernel_emu.h"

namespace {
#include KERNEL_BODY
}

static u32 key_by_bits(const u64 *row, int c0, int b) {
  u32 v = 0;
  for (int j = 0; j < b; ++j) v |= (u32)((row[(c0 + j) >> 6] >> ((c0 + j) & 63)) & 1) << j;
  return v;
}

int main() {
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
          const Lf1Window w = lf1_window(c0, b);
          if (lf1_key(row, w) != want) {
            printf("ncols %d c0 %d b %d: key %u, by bits %u\n", ncols, c0, b, lf1_key(row, w), want);
            return 1;
          }
          // only the words of the window: [first, last], none for b == 0
          const int first = c0 >> 6, last = b ? (c0 + b - 1) >> 6 : first - 1, held = last - first + 1;
          if (held < 0 || held > 2) {
            printf("ncols %d c0 %d b %d: %d words\n", ncols, c0, b, held);
            return 1;
          }
          u64 *part = new u64[held];
          for (int k = 0; k < held; ++k) part[k] = row[first + k];
          const u64 *shifted = reinterpret_cast<const u64 *>(reinterpret_cast<uintptr_t>(part) - 8 * (uintptr_t)first);
          if (lf1_key(shifted, w) != want) {
            printf("ncols %d c0 %d b %d: key of the window's words alone differs\n", ncols, c0, b);
            return 1;
          }
          delete[] part;
          ++cases;
        }
      delete[] row;
    }
  }
  printf("%ld keys ok\n", cases);
  return 0;
}
