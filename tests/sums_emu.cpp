// sums_emu.cpp -- the routines of the order of the subset sums (sums_max_c, sums_binomial, sums_rank, sums_unrank, sums_advance of
// m4ri-rust_amd/csrc/sums/sums_plan.h), cut out of the shipped file by tests/test_sums_helpers_cpu.py, on the CPU under the host
// compiler's address and undefined-behaviour sanitizers.  The word weight of the kernel is a shared helper: dev_words_emu.cpp.
//   binomials: against Pascal's rule in 128-bit arithmetic, up to the largest c of every level.
//   advance: for every p in 1 .. 4, n <= 14, every start rank and the strides 1, 2, 3, 64, 65, 1000, against `stride` single steps of a
//   successor written out here, against sums_unrank of the sum of the ranks, and the carry flag against "c_2 .. c_p changed".
//   unrank: around 2^31, 2^32 and 2^62 for every p, against sums_rank and against the neighbouring ranks (the successor of the
//   subset of rank r - 1 is the subset of rank r); the rest that is left for a rank at or past C(n, p).
#include "kernel_emu.h"

#define GF2_SUMS_FN inline

namespace {
#include KERNEL_BODY
}

typedef unsigned __int128 u128;

static u128 binomial128(unsigned c, int i) {
  u128 v = 1;
  for (int j = 1; j <= i; ++j) v = v * (u128)(c - (unsigned)(j - 1)) / (u128)j;  // C(c, j) from C(c, j - 1): exact
  return c < (unsigned)i ? 0 : v;
}

static long check_binomials() {
  long cases = 0;
  for (int i = 1; i <= 4; ++i) {
    std::vector<unsigned> cs;
    for (unsigned c = 0; c < 300; ++c) cs.push_back(c);
    const unsigned top = sums_max_c(i);
    for (unsigned d = 0; d < 50; ++d) cs.push_back(top - d);
    std::mt19937_64 rng(i);
    for (int k = 0; k < 2000; ++k) cs.push_back((unsigned)(rng() % ((u64)top + 1)));
    for (unsigned c : cs) {
      const u128 want = binomial128(c, i);
      if (want >> 63) {
        printf("C(%u, %d) does not stay below 2^63\n", c, i);
        return -1;
      }
      if ((u128)sums_binomial(c, i) != want) {
        printf("C(%u, %d): %llu\n", c, i, (unsigned long long)sums_binomial(c, i));
        return -1;
      }
      ++cases;
    }
    if (i >= 3 && !(binomial128(top + 1, i) >> 63)) {
      printf("sums_max_c(%d) is not the largest\n", i);
      return -1;
    }
  }
  return cases;
}

// the subset of the next rank, on the first p levels
static void successor(unsigned c[4], int p) {
  for (int i = 0; i < p; ++i) {
    if (i + 1 == p || c[i] + 1 < c[i + 1]) {
      ++c[i];
      return;
    }
    c[i] = (unsigned)i;
  }
}

static bool same(const unsigned a[4], const unsigned b[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }

static long check_advance() {
  const unsigned strides[] = {1, 2, 3, 64, 65, 1000};
  long cases = 0;
  for (int p = 1; p <= 4; ++p)
    for (unsigned n = (unsigned)p; n <= 14; ++n) {
      const u64 total = sums_binomial(n, p);
      for (u64 r = 0; r < total; ++r) {
        unsigned *start = new unsigned[4];  // a heap block of exactly the four levels
        if (sums_unrank(r, p, n, start) != 0 || sums_rank(start, p) != r) {
          printf("p %d n %u rank %llu: unrank\n", p, n, (unsigned long long)r);
          return -1;
        }
        for (int i = p; i < 4; ++i)
          if (start[i] != kSumsNone) return -1;
        for (unsigned stride : strides) {
          unsigned *c = new unsigned[4], walk[4], far[4];
          for (int i = 0; i < 4; ++i) c[i] = walk[i] = start[i];
          for (unsigned s = 0; s < stride; ++s) successor(walk, p);
          const bool carried = sums_advance(c, stride);
          sums_unrank(r + stride, p, 100000u, far);  // the rank does not depend on n
          bool moved = false;
          for (int i = 1; i < p; ++i) moved |= c[i] != start[i];
          if (!same(c, walk) || !same(c, far) || carried != moved) {
            printf("p %d n %u rank %llu + %u: advance gives %u %u %u %u (carry %d), single steps %u %u %u %u\n", p, n, (unsigned long long)r,
                   stride, c[0], c[1], c[2], c[3], (int)carried, walk[0], walk[1], walk[2], walk[3]);
            return -1;
          }
          delete[] c;
          ++cases;
        }
        delete[] start;
      }
    }
  return cases;
}

static long check_unrank_at_large_ranks() {
  long cases = 0;
  const u64 around[] = {1ull << 31, 1ull << 32, 1ull << 62};
  for (int p = 1; p <= 4; ++p) {
    const unsigned n = p <= 2 ? kSumsNone : sums_max_c(p) + 1;  // every c that the routines take: C(n, p) passes 2^62, the ranks around it are inside
    const u128 total128 = binomial128(n, p);
    const u64 total = total128 >> 63 ? ~0ull : (u64)total128;   // p = 1: 2^32 - 1; else past every rank below
    std::vector<u64> ranks = {0, 1, total / 2, p == 1 ? total - 1 : (1ull << 62) + (1ull << 61)};
    for (u64 a : around)
      for (long long d = -70; d <= 70; ++d) ranks.push_back(a + (u64)d);
    for (u64 r : ranks) {
      unsigned c[4], prev[4];
      const u64 left = sums_unrank(r, p, n, c);
      if (r >= total) {  // the last subset, and what is left says that the rank is outside
        if (left != r - (total - 1) || c[p - 1] != n - 1) {
          printf("p %d rank %llu >= C(n, p): left %llu\n", p, (unsigned long long)r, (unsigned long long)left);
          return -1;
        }
        ++cases;
        continue;
      }
      bool ok = left == 0 && sums_rank(c, p) == r && c[p - 1] < n;
      for (int i = 0; i + 1 < p; ++i) ok = ok && c[i] < c[i + 1];
      if (ok && r > 0) {
        sums_unrank(r - 1, p, n, prev);
        successor(prev, p);
        ok = same(prev, c);
        unsigned step[4];
        sums_unrank(r - 1, p, n, step);
        sums_advance(step, 1);
        ok = ok && same(step, c);
        if (r >= 256) {  // a workgroup's stride across the rank
          sums_unrank(r - 256, p, n, step);
          sums_advance(step, 256);
          ok = ok && same(step, c);
        }
      }
      if (!ok) {
        printf("p %d rank %llu: %u %u %u %u\n", p, (unsigned long long)r, c[0], c[1], c[2], c[3]);
        return -1;
      }
      ++cases;
    }
  }
  return cases;
}

int main() {
  const long binomials = check_binomials();
  if (binomials < 0) return 1;
  printf("%ld binomials ok\n", binomials);
  const long advances = check_advance();
  if (advances < 0) return 1;
  printf("%ld advances ok\n", advances);
  const long unranks = check_unrank_at_large_ranks();
  if (unranks < 0) return 1;
  printf("%ld unranks ok\n", unranks);
  return 0;
}
