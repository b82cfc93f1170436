// gather_emu.cpp -- runs the row-gather kernel of m4ri-rust_amd/csrc/gather/gf2_gather.hip thread by thread on the CPU
// (tests/test_gather_kernels_cpu.py cuts its shipped text, its helper and its launcher out of the .hip file with tests/kernel_text.py
// into KERNEL_BODY and builds this file with the host compiler and its address / undefined-behaviour sanitizers; the stand-ins for the
// HIP names are tests/kernel_emu.h).  The rules are those of kernels_emu.cpp: every buffer is an exact malloc that ends with the last
// word of the operand's last row (the index array with its last int), bases are 16-byte aligned and 8 bytes off, ld runs over width,
// width + 1 and width + 2, content is random, the expectation comes from plain loops written here, and the WHOLE destination buffer
// is compared.  The launcher is what is called, so its choice of 16-byte pieces is what the alignment check judges.
#include <climits>

#include "kernel_emu.h"
#include KERNEL_BODY

static std::mt19937_64 rng(20241019);

#define FAIL(...)                    \
  do {                               \
    printf("MISMATCH " __VA_ARGS__); \
    printf("\n");                    \
    exit(1);                         \
  } while (0)

template <typename T>
struct Exact {  // n elements, `off` bytes behind a 16-byte boundary, random content, the red zone right behind the last one
  char *raw;
  T *p;
  long long n;
  Exact(long long n_, int off_bytes = 0) : n(n_) {
    raw = (char *)malloc((size_t)n_ * sizeof(T) + off_bytes);
    if ((uintptr_t)raw & 15) { printf("malloc not 16-aligned\n"); exit(2); }
    p = (T *)(raw + off_bytes);
    unsigned char *b = (unsigned char *)p;
    for (size_t i = 0; i < (size_t)n_ * sizeof(T); ++i) b[i] = (unsigned char)rng();
  }
  Exact(const Exact &) = delete;
  ~Exact() { free(raw); }
};
static long long span(long long rows, long long ld, long long width) { return rows <= 0 ? 0 : (rows - 1) * ld + width; }
static u64 lastmask(long long bits) { return (bits & 63) ? ((1ull << (bits & 63)) - 1) : ~0ull; }

int main() {
  const int kCols[] = {1, 63, 64, 65, 128, 191};
  const int kShapes[][2] = {{1, 1}, {5, 3}, {300, 7}, {4, 0}};  // D rows, S rows (0: S is null, every index is out of range)
  long cases = 0;
  for (int ncols : kCols)
    for (auto &shape : kShapes)
      for (int g = 0; g < 3 * 3 * 2 * 2; ++g)
        for (int accumulate = 0; accumulate < 2; ++accumulate)
          for (int pattern = 0; pattern < 2; ++pattern) {  // 0: every index in range; 1: in range, -1, nrows, INT_MIN, INT_MAX mixed
            const int dn = shape[0], sn = shape[1];
            const long long nw = (ncols + 63) / 64, ldd = nw + g % 3, lds_ = nw + g / 3 % 3;
            const int od = g / 9 & 1, os = g / 18 & 1;
            Exact<u64> D(span(dn, ldd, nw), 8 * od), S(span(sn, lds_, nw), 8 * os);
            Exact<int> idx(dn), bad(1);
            bad.p[0] = 0;
            int want_bad = 0;
            for (int i = 0; i < dn; ++i) {
              const int special[] = {-1, sn, INT_MIN, INT_MAX, sn + 1, -2};
              const unsigned pick = (unsigned)(rng() % 12);
              idx.p[i] = (sn > 0 && (pattern == 0 || pick >= 6)) ? (int)(rng() % (unsigned)sn) : special[pick % 6];
              if (dn >= 5 && pattern == 1 && i < 6) idx.p[i] = i == 4 && sn > 0 ? 0 : special[i];  // every special value at least once
              const bool ok = idx.p[i] >= 0 && idx.p[i] < sn;
              if (!ok && idx.p[i] != -1) want_bad = 1;
            }
            std::vector<u64> want(D.p, D.p + D.n);
            for (int i = 0; i < dn; ++i) {
              const bool ok = idx.p[i] >= 0 && idx.p[i] < sn;
              if (!ok && accumulate) continue;
              for (long long w = 0; w < nw; ++w) {
                u64 v = ok ? S.p[(long long)idx.p[i] * lds_ + w] : 0ull;
                if (w == nw - 1) v &= lastmask(ncols);
                want[i * ldd + w] = accumulate ? (want[i * ldd + w] ^ v) : v;
              }
            }
            const std::vector<int> idx_before(idx.p, idx.p + dn);
            if (gf2k_gather_rows(D.p, ldd, sn ? S.p : nullptr, lds_, dn, sn, ncols, idx.p, accumulate, bad.p, nullptr) != hipSuccess)
              FAIL("status");
            for (long long i = 0; i < D.n; ++i)
              if (D.p[i] != want[i])
                FAIL("gather_rows (cols %d, %d <- %d rows, g %d, acc %d, pattern %d): word %lld is %016llx, want %016llx", ncols, dn, sn, g,
                     accumulate, pattern, i, (unsigned long long)D.p[i], (unsigned long long)want[i]);
            if (bad.p[0] != want_bad) FAIL("bad is %d, want %d (cols %d, %d <- %d rows, pattern %d)", bad.p[0], want_bad, ncols, dn, sn, pattern);
            if (!std::equal(idx_before.begin(), idx_before.end(), idx.p)) FAIL("the index array changed");
            // without a flag to write to, the same call must not touch one
            if (pattern == 1 && g == 0 &&
                gf2k_gather_rows(D.p, ldd, sn ? S.p : nullptr, lds_, dn, sn, ncols, idx.p, accumulate, nullptr, nullptr) != hipSuccess)
              FAIL("status without a flag");
            ++cases;
          }
  // empty shapes launch nothing and touch nothing
  if (gf2k_gather_rows(nullptr, 0, nullptr, 0, 0, 5, 64, nullptr, 0, nullptr, nullptr) != hipSuccess) FAIL("empty rows");
  if (gf2k_gather_rows(nullptr, 0, nullptr, 0, 5, 5, 0, nullptr, 0, nullptr, nullptr) != hipSuccess) FAIL("empty columns");
  printf("gf2_gather_rows_kernel: %ld cases ok\n", cases);
  printf("all ok, %ld threads\n", g_threads);
  return 0;
}
