// blocks_emu.cpp -- runs the block-copy kernel of m4ri-rust_amd/csrc/gf2_blocks.hip thread by thread on the CPU (tests/test_blocks_kernel_cpu.py
// builds this file with the host compiler and its address / undefined-behaviour sanitizers).  The kernel text is included as it is, behind
// the stand-ins of tests/kernel_emu.h for the few HIP names it uses.  Every buffer ends with the last word of the rectangle's last row, so an access to a word that
// holds no bit of the rectangle -- which a GPU test could only show by faulting -- is an error report here.  Results are compared bit by bit
// over the whole destination buffer.  KERNEL_BODY: the .hip file without its #include lines.
#include "kernel_emu.h"
#include KERNEL_BODY

static int getbit(const u64 *p, long long ld, long long r, long long c) { return (p[r * ld + (c >> 6)] >> (c & 63)) & 1; }

int main() {
  std::mt19937_64 rng(12345);
  long cases = 0;
  const int offs[] = {0, 1, 31, 32, 33, 63, 5, 59, 7};
  const int widths[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 200, 513, 1100};
  for (int so : offs) for (int doo : offs) for (int nc : widths) for (int variant = 0; variant < 8; ++variant) {
    const int acc = variant & 1, zt = (variant >> 1) & 1 && !acc;
    const int sx = (variant >> 2) & 1, dx = (variant >> 1) & 1;
    const int nrows = 1 + (int)(rng() % 5) + (nc < 10 ? 300 : 0);
    const long long sc = so + 64 * sx, dc = doo + 64 * dx, sr = rng() % 3, dr = rng() % 3;
    // tight geometry: the rectangle ends with the last word of the last row of each buffer; ld odd or even
    const long long s_w = (sc + nc + 63) / 64, d_w = (dc + nc + 63) / 64;
    const long long lds = s_w + rng() % 3, ldd = d_w + rng() % 3;
    const long long s_words = (sr + nrows - 1) * lds + s_w, d_words = (dr + nrows - 1) * ldd + d_w;
    // base alignment: 16 bytes or 8 bytes off
    const int s_off = rng() & 1, d_off = rng() & 1;
    // exact sizes: the sanitizer's red zone starts right behind the rectangle's last word
    u64 *sbuf = (u64 *)malloc((size_t)(s_words + s_off) * 8);
    u64 *dbuf = (u64 *)malloc((size_t)(d_words + d_off) * 8);
    if (((uintptr_t)sbuf & 15) || ((uintptr_t)dbuf & 15)) { printf("malloc not 16-aligned\n"); return 2; }
    u64 *S = sbuf + s_off, *D = dbuf + d_off;
    for (long long i = 0; i < s_words; ++i) S[i] = rng();
    for (long long i = 0; i < d_words; ++i) D[i] = rng();
    std::vector<u64> d0(D, D + d_words);
    gf2k_copy_block(D, ldd, dr, dc, S, lds, sr, sc, nrows, nc, acc, zt, nullptr);
    // expected, bit by bit over the whole D buffer
    for (long long w = 0; w < d_words; ++w) {
      const long long r = w / ldd, cw = w % ldd;
      for (int b = 0; b < 64; ++b) {
        const long long c = cw * 64 + b, i = r - dr, j = c - dc;
        int want = (d0[w] >> b) & 1;
        if (cw < d_w && i >= 0 && i < nrows && j >= 0 && j < nc) {
          const int sbit = getbit(S, lds, sr + i, sc + j);
          want = acc ? want ^ sbit : sbit;
        } else if (zt && cw == d_w - 1 && i >= 0 && i < nrows && j >= nc) want = 0;
        if (((D[w] >> b) & 1) != want) {
          printf("MISMATCH so=%d do=%d nc=%d variant=%d row=%lld col=%lld\n", so, doo, nc, variant, r, c);
          return 1;
        }
      }
    }
    free(sbuf); free(dbuf);
    ++cases;
  }
  // a tall one: 2^20 + 1 rows x 65 columns at offsets (7, 0): the grid shape
  {
    const int nrows = (1 << 20) + 1, nc = 65;
    std::vector<u64> S((size_t)nrows * 2), D((size_t)nrows * 2), d0;
    for (auto &x : S) x = rng();
    for (auto &x : D) x = rng();
    d0 = D;
    gf2k_copy_block(D.data(), 2, 0, 0, S.data(), 2, 0, 7, nrows, nc, 0, 0, nullptr);
    for (long long r = 0; r < nrows; ++r) {
      const u64 w0 = (S[r * 2] >> 7) | (S[r * 2 + 1] << 57), w1 = ((S[r * 2 + 1] >> 7) & 1) | (d0[r * 2 + 1] & ~1ull);
      if (D[r * 2] != w0 || D[r * 2 + 1] != w1) { printf("tall mismatch row %lld\n", r); return 1; }
    }
    printf("tall ok, grid %u x %u block %u x %u\n", gridDim.x, gridDim.y, blockDim.x, blockDim.y);
  }
  printf("%ld cases ok, %ld threads emulated\n", cases, g_threads);
  return 0;
}
