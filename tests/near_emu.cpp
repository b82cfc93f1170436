// near_emu.cpp -- the word-level helpers of the Hamming-distance search (near_first_word, near_end_word, near_chunk_begin,
// near_chunk_end, near_cell and near_plan of m4ri-rust_amd/csrc/near/near_plan.h; gf2_word_mask of gf2_dev_words.h, which they use;
// near_in_window, near_excluded, near_tile_class, near_pack_key, near_chunk_key, near_wide_key, near_key_dist, near_key_index, near_weight, near_row_weight and
// near_tile_row of gf2_near.hip; cut out of the shipped files by tests/test_near_helpers_cpu.py) on the CPU under the host compiler's
// address and undefined-behaviour sanitizers.
//   the words and masks of a range: for every [wc0, wc1) of a row of ncols bits, [first, end) are exactly the words that hold a column
//   of the range, the masks of those words are exactly the range's bits, and the masked popcounts sum to the bit-by-bit count.
//   the weight of a pair: near_row_weight on rows in heap blocks of exactly the row's words (a read behind the row is an error of the
//   address sanitizer), and near_weight<W> on the masked words through near_tile_row<W> (a tile in a heap block of its own).
//   the window: for every range and every 0 <= wlo <= whi <= width + 2, and whi = 2^31 - 1.
//   the keys: packing, the order of the packed keys against (weight, row), the chunk key and its parts, also past 2^31 rows.
//   the flags and the classes of tiles against a loop over the pairs; chunk bounds; cells past 2^32; the plan's chunks cover B.
#include "kernel_emu.h"
#include "near_plan.h"  // m4ri-rust_amd/csrc/near, as shipped: plain host arithmetic

struct alignas(16) ulonglong2 {
  unsigned long long x, y;
};
#define GF2_NEAR_OFF_DIAGONAL 1
#define GF2_NEAR_UPPER 2

namespace {
#include KERNEL_BODY
}

#define FAIL(...)          \
  do {                     \
    printf(__VA_ARGS__);   \
    printf("\n");          \
    return 1;              \
  } while (0)

template <int W>
int tile_weights(const std::vector<u64> &a, const std::vector<u64> &p, int nw, int wc0, int wc1, int want) {
  const long long first = near_first_word(wc0, wc1), end = near_end_word(wc0, wc1);
  if (end - first > W) return 0;  // not this kernel's range
  const int rows = 4;  // a multiple of 16 bytes for every W; row 1 is the one that is read
  u64 *tile = static_cast<u64 *>(aligned_alloc(16, 8 * W * rows));
  u64 am[W];
  for (int k = 0; k < W; ++k) {
    const bool in = k < end - first;
    am[k] = in ? a[first + k] & gf2_word_mask(first + k, wc0, wc1) : 0;
    for (int r = 0; r < rows; ++r) tile[r * W + k] = in && r == 1 ? p[first + k] & gf2_word_mask(first + k, wc0, wc1) : 0;
  }
  u64 b[W];
  near_tile_row<W>(tile, 1, b);
  const int got = near_weight<W>(am, b);
  free(tile);
  (void)nw;
  return got == want ? 1 : -1;
}

int main() {
  const int widths[] = {1, 63, 64, 65, 130, 1100};
  std::mt19937_64 rng(2029);
  long ranges = 0, windows = 0, weights = 0, keys = 0, classes = 0;
  for (int ncols : widths) {
    const int nw = (ncols + 63) >> 6;
    const int step = ncols > 200 ? 37 : 1;  // the wide row: a sample of the ranges
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<u64> a(nw), p(nw);
      for (int k = 0; k < nw; ++k) {
        a[k] = rep == 1 ? ~0ull : rng();
        p[k] = rep == 1 ? 0ull : rep == 2 ? a[k] ^ (0xAAAAAAAAAAAAAAAAull >> (k & 1)) : rng();  // excess bits of the last word are dirty
      }
      u64 *ha = static_cast<u64 *>(malloc(8 * nw)), *hp = static_cast<u64 *>(malloc(8 * nw));  // exactly nw words
      std::copy(a.begin(), a.end(), ha);
      std::copy(p.begin(), p.end(), hp);
      for (int wc0 = 0; wc0 <= ncols; wc0 += step)
        for (int wc1 = wc0; wc1 <= ncols; wc1 += step) {
          int want = 0;
          for (int c = wc0; c < wc1; ++c) want += (int)(((a[c >> 6] ^ p[c >> 6]) >> (c & 63)) & 1);
          const long long first = near_first_word(wc0, wc1), end = near_end_word(wc0, wc1);
          if (first < 0 || first > end || end > nw) FAIL("ncols %d [%d, %d): words [%lld, %lld)", ncols, wc0, wc1, first, end);
          int got = 0;
          for (long long k = 0; k < nw; ++k) {
            u64 m = 0;
            for (int c = wc0; c < wc1; ++c)
              if ((c >> 6) == k) m |= 1ull << (c & 63);
            if (gf2_word_mask(k, wc0, wc1) != m) FAIL("ncols %d [%d, %d): the mask of word %lld", ncols, wc0, wc1, k);
            if ((m != 0) != (k >= first && k < end)) FAIL("ncols %d [%d, %d): word %lld and [%lld, %lld)", ncols, wc0, wc1, k, first, end);
            got += __popcll((a[k] ^ p[k]) & gf2_word_mask(k, wc0, wc1));
          }
          if (got != want) FAIL("ncols %d [%d, %d): weight %d over the masked words, by bits %d", ncols, wc0, wc1, got, want);
          if (near_row_weight(ha, hp, first, end, wc0, wc1) != want) FAIL("ncols %d [%d, %d): near_row_weight", ncols, wc0, wc1);
          ++ranges;
          const int t[5] = {tile_weights<1>(a, p, nw, wc0, wc1, want), tile_weights<2>(a, p, nw, wc0, wc1, want),
                            tile_weights<4>(a, p, nw, wc0, wc1, want), tile_weights<8>(a, p, nw, wc0, wc1, want),
                            tile_weights<16>(a, p, nw, wc0, wc1, want)};
          for (int v : t) {
            if (v < 0) FAIL("ncols %d [%d, %d): near_weight over a tile row", ncols, wc0, wc1);
            weights += v;
          }
          const int width = wc1 - wc0;
          if (ncols <= 130)
            for (int wlo = 0; wlo <= width + 2; ++wlo) {
              for (int whi = wlo; whi <= width + 2; ++whi) {
                if (near_in_window(want, wlo, (u32)whi - (u32)wlo) != (wlo <= want && want <= whi))
                  FAIL("ncols %d [%d, %d) weight %d window [%d, %d]", ncols, wc0, wc1, want, wlo, whi);
                ++windows;
              }
              if (near_in_window(want, wlo, 0x7FFFFFFFu - (u32)wlo) != (wlo <= want)) FAIL("a window up to 2^31 - 1");
            }
        }
      free(ha);
      free(hp);
    }
  }
  // the keys: a lower (weight, row) is a lower key; the chunk key gives both back, also for rows past 2^31 - 2^20
  const long long j0s[] = {0, 512, (1ll << 31) - (1ll << 20)};
  for (int w : {0, 1, 63, 64, 500, 1023, 1024})
    for (u32 jrel : {0u, 1u, 511u, (1u << 20) - 1})
      for (long long j0 : j0s) {
        const u32 key = near_pack_key(w, jrel);
        if (key == ~0u) FAIL("a key equals the empty key");
        const u64 wide = near_chunk_key(key, j0);
        if (near_key_dist(wide) != w || (long long)(u32)near_key_index(wide) != j0 + jrel) FAIL("key (%d, %u) at %lld", w, jrel, j0);
        if (wide != near_wide_key(w, j0 + jrel)) FAIL("the chunk key is not the wide key");
        for (int w2 : {0, 1, 64, 1024})
          for (u32 j2 : {0u, 2u, (1u << 20) - 1}) {
            const bool less = w < w2 || (w == w2 && jrel < j2);
            if ((key < near_pack_key(w2, j2)) != less) FAIL("the order of the keys (%d, %u) and (%d, %u)", w, jrel, w2, j2);
            ++keys;
          }
      }
  if (near_chunk_key(~0u, 77) != ~0ull || near_key_dist(~0ull) != -1 || near_key_index(~0ull) != -1) FAIL("the empty key");
  if (near_key_dist(near_wide_key(0x7FFFFFFF, 0x7FFFFFFE)) != 0x7FFFFFFF || near_key_index(near_wide_key(5, 0x7FFFFFFE)) != 0x7FFFFFFE)
    FAIL("a wide key at the largest weight and row");
  // the flags, and the class of a tile against a loop over its pairs
  for (int flags = 0; flags < 4; ++flags)
    for (long long r0 : {0ll, 4ll, 8ll})
      for (long long t0 = 0; t0 < 14; ++t0)
        for (long long t1 = t0 + 1; t1 < 16; ++t1) {
          const long long r1 = r0 + 4;
          int some = 0, all = 1;
          for (long long i = r0; i < r1; ++i)
            for (long long j = t0; j < t1; ++j) {
              const int ex = (flags & 2) ? j <= i : (flags & 1) ? j == i : 0;
              if (near_excluded(i, j, flags) != ex) FAIL("near_excluded(%lld, %lld, %d)", i, j, flags);
              some |= ex;
              all &= ex;
            }
          const int cls = near_tile_class(r0, r1, t0, t1, flags);
          if ((cls == 0 && some) || (cls == 2 && !all) || cls < 0 || cls > 2) FAIL("tile class %d of [%lld, %lld) x [%lld, %lld) flags %d", cls, r0, r1, t0, t1, flags);
          if ((flags & 2) && all && cls != 2) FAIL("a tile without admitted pairs is not skipped");
          ++classes;
        }
  // chunk bounds and cells: 64-bit throughout
  if (near_chunk_begin(2047, 1 << 20) != 2047ll << 20 || near_chunk_end(2047, 1 << 20, 0x7FFFFFFF) != 0x7FFFFFFF) FAIL("the last chunk");
  if (near_chunk_end(3, 512, 5000) != 2048 || near_chunk_end(9, 512, 5000) != 5000) FAIL("chunk ends");
  if (near_cell(0x7FFFFFFE, 2048, 2047) != 0x7FFFFFFEll * 2048 + 2047 || near_cell(3000000, 2048, 5) <= 1ll << 32) FAIL("cells past 2^32");
  long plans = 0;
  for (long long na : {0ll, 1ll, 5ll, 511ll, 512ll, 513ll, 700ll, 65536ll, 1ll << 20, 0x7FFFFFFFll})
    for (long long nb : {0ll, 1ll, 63ll, 64ll, 65ll, 600ll, 20000ll, 70000ll, 1ll << 20, (1ll << 20) + 1, 0x7FFFFFFFll})
      for (long long words : {0ll, 1ll, 2ll, 3ll, 5ll, 16ll, 17ll}) {
        const NearPlan p = near_plan(na, nb, 64 * 20, 64, 64 + 64 * words);
        const long long unit = p.kernel ? p.tile_rows : kNearWideUnit;
        if (p.kernel < 0 || p.words != words || p.chunks < 1 || p.chunks > 65535 || p.chunk_rows % unit || p.chunk_rows > kNearMaxChunkRows)
          FAIL("plan %lld %lld %lld", na, nb, words);
        if (p.kernel && (p.kernel < words || p.tile_rows * 8 * p.kernel != kNearTileBytes)) FAIL("plan: the tile");
        if (nb > 0 && (p.chunks * p.chunk_rows < nb || (p.chunks - 1) * p.chunk_rows >= nb)) FAIL("plan: the chunks do not cover B exactly");
        if (p.row_blocks * p.block_rows < na || p.scratch < 8 * (na * p.chunks + 1)) FAIL("plan: the rows or the scratch");
        ++plans;
      }
  if (near_plan(1, 1, 10, 5, 4).kernel != -1 || near_plan(1, 1, 10, 0, 11).kernel != -1 || near_plan(-1, 1, 10, 0, 1).kernel != -1) FAIL("bad plans");
  printf("%ld ranges ok\n%ld tile weights ok\n%ld windows ok\n%ld keys ok\n%ld classes ok\n%ld plans ok\n", ranges, weights, windows, keys, classes, plans);
  return 0;
}
