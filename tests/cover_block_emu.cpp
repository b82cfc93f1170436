// cover_block_emu.cpp -- the block reader and decoder of the covering-code kernels (cover_syn_bit / cover_block of
// m4ri-rust_amd/csrc/cover/gf2_cover.hip) and the host routines behind the codes (gf2_cover_code_named / gf2_cover_leaders of
// cover_host.cpp), cut out of the shipped files by tests/test_cover_block_cpu.py, on the CPU under the host compiler's address and
// undefined-behaviour sanitizers.  Every row lives in a heap block that ENDS with the last word of the block's window; a second run
// gives the helper a heap block that holds ONLY the words with a bit of the block.  Every table is a heap block of exactly 2^r words
// (none for a code without one).  A read of any other word is a sanitizer report.  What comes out is printed, and the test compares it
// with tests/cover_ref.py.
#include "kernel_emu.h"
#define __host__
#include "cover/cover_plan.h"

#include HOST_BODY

namespace {
#include KERNEL_BODY
}

static u64 splitmix64(u64 seed, u64 t) {
  u64 z = seed + (t + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main() {
  const int kReps = 4, kWords = 3;
  std::vector<gf2_cover_code> codes;
  const int named[][2] = {{GF2_COVER_IDENTITY, 1},  {GF2_COVER_DROP, 1},  {GF2_COVER_HAMMING, 3}, {GF2_COVER_GOLAY23, 0}, {GF2_COVER_HAMMING, 5},
                          {GF2_COVER_IDENTITY, 32}, {GF2_COVER_DROP, 32}, {GF2_COVER_REPETITION, 13}};
  for (const auto &nm : named) {
    gf2_cover_code c;
    if (gf2_cover_code_named(nm[0], nm[1], &c)) return 2;
    codes.push_back(c);
  }
  gf2_cover_code wide;  // [32, 22]: a table code that fills the word
  memset(&wide, 0, sizeof wide);
  wide.n = 32;
  wide.k = 22;
  for (int t = 0; t < 10; ++t) wide.h[t] = (u32)(splitmix64(7, t) & ((1u << 22) - 1)) | (1u << (22 + t));
  codes.push_back(wide);
  long cases = 0;
  for (size_t ci = 0; ci < codes.size(); ++ci) {
    const gf2_cover_code &c = codes[ci];
    const int r = c.n - c.k;
    const bool table = cover_has_table(c);
    u32 *leaders = table ? new u32[1u << r] : nullptr;
    int radius = -1;
    u32 one[1] = {0xDEADBEEF};
    if (gf2_cover_leaders(&c, table ? leaders : one, &radius)) return 3;
    if (!table && one[0] != (c.k ? 0u : 0xDEADBEEF)) return 4;
    printf("code %zu %d %d radius %d\n", ci, c.n, c.k, radius);
    if (table)
      for (u32 s = 0; s < (1u << r); ++s) printf("L %zu %u %u\n", ci, s, leaders[s]);
    u32 *h = table ? new u32[GF2_COVER_MAX_R] : nullptr;  // the check rows as the kernel has them: twelve words; none where none is read
    if (table) memcpy(h, c.h, sizeof c.h);
    for (int o = 0; o < 128; ++o) {
      const int first = o >> 6, last = (o + c.n - 1) >> 6, held = last - first + 1;
      if (held < 1 || held > 2) return 5;
      for (int rep = 0; rep < kReps; ++rep) {
        u64 *row = new u64[last + 1];  // ends with the last word of the block
        for (int k = 0; k <= last; ++k) row[k] = splitmix64(2026, (u64)rep * kWords + k);
        const CoverBlock b = cover_block(row, o, c.n, c.k, h, leaders);
        u64 *part = new u64[held];     // only the words of the block
        for (int k = 0; k < held; ++k) part[k] = row[first + k];
        const CoverBlock b2 = cover_block(part, o - 64 * first, c.n, c.k, h, leaders);
        if (b.msg != b2.msg || b.wt != b2.wt) {
          printf("code %zu o %d rep %d: the block's words alone decode differently\n", ci, o, rep);
          return 1;
        }
        printf("B %zu %d %d %u %d\n", ci, o, rep, b.msg, b.wt);
        delete[] part;
        delete[] row;
        ++cases;
      }
    }
    delete[] h;
    delete[] leaders;
  }
  printf("%ld blocks ok\n", cases);
  return 0;
}
