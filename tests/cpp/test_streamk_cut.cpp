// The stream-K cut and the variant table the launch planner and the tile-kernel launcher share (m4ri-rust_amd/csrc/gf2_variants.h),
// checked exhaustively over small ranges.  Includes nothing but that header: compiling this file with g++ shows that it needs no HIP.
#include <cstdio>

#include "../../m4ri-rust_amd/csrc/gf2_variants.h"

static long long failures = 0;
#define CHECK(cond)                                                                                                        \
  do {                                                                                                                     \
    if (!(cond) && failures++ < 20) std::printf("FAILED %s: T=%lld Q=%lld n_rem=%lld want=%lld\n", #cond, T, Q, n_rem, want); \
  } while (0)

int main() {
  long long cases = 0, cut_cases = 0;
  for (long long T = 1; T <= 300; ++T)
    for (long long Q = 1; Q <= 40; ++Q) {
      const long long n_rems[4] = {1, T / 2, T % 256, T}, wants[5] = {1, 3, 256, T + 1, 3 * T + 2};
      for (long long n_rem : n_rems)
        for (long long want : wants) {
          const gf2_streamk_cut c = gf2_streamk_cut_of(T, Q, n_rem, want);
          ++cases;
          // nothing would be cut: no tiles were asked for, or the segment length that gives `want` segments is a whole tile or more
          const bool nothing_cut = n_rem <= 0 || (n_rem * Q + want - 1) / want >= Q;
          CHECK((c.n_rem == 0) == nothing_cut);
          if (c.n_rem == 0) {
            CHECK(c.nseg == 0 && c.seg == 0);
            continue;
          }
          ++cut_cases;
          CHECK(c.n_rem == n_rem);  // (n_rem <= T in these ranges)
          CHECK(1 <= c.seg && c.seg <= Q);
          CHECK((c.nseg - 1) * c.seg < c.n_rem * Q && c.n_rem * Q <= c.nseg * c.seg);
          CHECK(c.seg < Q && c.nseg > c.n_rem);  // something IS cut: more segments than tiles
          for (int cfg = 9; cfg <= 12; ++cfg) {  // the four row groups: two slots of 512 RG rows x 8 words per segment
            const gf2_variant v = gf2_variant_of(cfg);
            const int rg = 8 >> (cfg - 9);
            CHECK(v.v8_rg == rg && v.rows == 512 * rg && v.cols == 512 && v.reads_packed && v.shipped);
            CHECK(gf2_streamk_words(v, c.nseg) == 2ll * c.nseg * 512 * rg * 8);
          }
        }
    }
  {  // a request beyond the launch is clamped to it; want < 1 means 256
    const long long T = 5, Q = 7, n_rem = 9, want = 0;
    const gf2_streamk_cut c = gf2_streamk_cut_of(T, Q, n_rem, want), d = gf2_streamk_cut_of(T, Q, T, 256);
    CHECK(c.n_rem == T && c.nseg == d.nseg && c.seg == d.seg);
    CHECK(gf2_streamk_words(gf2_variant_of(7), 10) == 0 && !gf2_variant_of(7).reads_packed && !gf2_variant_of(20).reads_packed);
    CHECK(gf2_variant_of(8).reads_packed && gf2_variant_of(8).rows == 2048 && gf2_variant_of(8).cols == 1024);
    CHECK(gf2_variant_of(7).rows == 1024 && gf2_variant_of(7).cols == 2048 && gf2_variant_of(20).rows == 256 && gf2_variant_of(20).cols == 2048);
    CHECK(!gf2_variant_of(13).shipped && !gf2_variant_of(0).shipped && gf2_variant_of(81).shipped && gf2_variant_of(82).shipped);
  }
  std::printf("%lld cases, %lld of them cut, %lld failures\n", cases, cut_cases, failures);
  return failures || cut_cases == 0 || cut_cases == cases ? 1 : 0;
}
