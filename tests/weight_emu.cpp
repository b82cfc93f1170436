// weight_emu.cpp -- runs the narrow row-weight kernel of m4ri-rust_amd/csrc/weight/gf2_weight.hip thread by thread on the CPU
// (tests/test_weight_kernels_cpu.py cuts its shipped text, its helpers and its launcher out of the .hip file with
// tests/kernel_text.py into KERNEL_BODY and builds this file with the host compiler and its address / undefined-behaviour
// sanitizers; the stand-ins for the HIP names are tests/kernel_emu.h).  The rules are those of gather_emu.cpp: the operand is an exact
// malloc that ends with the last word of its last row, `weights` one that ends with its last int, bases are 16-byte aligned and 8
// bytes off, ld runs over width, width + 1 and width + 2, the expectation comes from plain loops written here.  A read of a pad word
// or of a word past the row width at the end of the buffer, a misaligned 16-byte load and a store past `weights` are sanitizer
// reports.  The launcher is what is called, so its choice of 16-byte loads is what the alignment check judges.
#include "kernel_emu.h"
#include KERNEL_BODY

static std::mt19937_64 rng(20261019);

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
  const int kCols[] = {1, 63, 64, 65, 128, 129, 192, 255, 256};  // up to the variant's limit of four words
  const int kRows[] = {1, 5, 64, 65};
  long cases = 0;
  for (int ncols : kCols)
    for (int nrows : kRows)
      for (int g = 0; g < 3 * 2; ++g)          // ld = width, width + 1, width + 2; base on a 16-byte boundary and 8 bytes off
        for (int content = 0; content < 3; ++content) {  // random; all ones; all ones with the excess bits of the last word set too
          const long long nw = (ncols + 63) / 64, ld = nw + g % 3;
          const int off = g / 3;
          Exact<u64> A(span(nrows, ld, nw), 8 * off);
          Exact<int> W(nrows);
          std::vector<int> want(nrows);
          for (int r = 0; r < nrows; ++r) {
            int c = 0;
            for (long long w = 0; w < nw; ++w) {
              u64 &x = A.p[r * ld + w];
              if (content >= 1) x = ~0ull;
              if (content == 1 && w == nw - 1) x &= lastmask(ncols);
              c += __builtin_popcountll(w == nw - 1 ? x & lastmask(ncols) : x);
            }
            want[r] = c;
            if (content >= 1 && c != ncols) FAIL("the expectation itself");
          }
          const std::vector<u64> before(A.p, A.p + A.n);
          if (gf2k_weight_rows_narrow(A.p, ld, nrows, ncols, W.p, nullptr) != hipSuccess) FAIL("status");
          for (int r = 0; r < nrows; ++r)
            if (W.p[r] != want[r])
              FAIL("row weights (%d x %d, ld %lld, off %d, content %d): row %d is %d, want %d", nrows, ncols, ld, off, content, r, W.p[r],
                   want[r]);
          if (!std::equal(before.begin(), before.end(), A.p)) FAIL("the operand changed");
          ++cases;
        }
  // empty shapes launch nothing and touch nothing
  if (gf2k_weight_rows_narrow(nullptr, 0, 0, 64, nullptr, nullptr) != hipSuccess) FAIL("no rows");
  if (gf2k_weight_rows_narrow(nullptr, 0, 5, 0, nullptr, nullptr) != hipSuccess) FAIL("no columns");
  printf("gf2_weight_rows_narrow_kernel: %ld cases ok\n", cases);
  printf("all ok, %ld threads\n", g_threads);
  return 0;
}
