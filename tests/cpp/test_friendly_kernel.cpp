// BinMatrix::kernel() of include/m4ri_friendly.hpp (mzd_kernel_left_pluq): A * K == 0, K's rows at the free columns are the
// identity, the receiver stays as it was, full column rank gives no basis.
// usage: test_friendly_kernel     exit code 0 = all assertions held (needs a device: the entry points have no fallback)
#include <cstdio>

#include "m4ri_friendly.hpp"
using namespace m4ri_friendly;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool is_zero(const BinMatrix &m) { return mzd_is_zero(m.raw()) != 0; }

int main() {
  {  // [I | R] with R 40 x 90: pivots first, so K = [R; I]
    BinMatrix R = BinMatrix::random(40, 90), A = BinMatrix::identity(40).augmented(R), before = A;
    std::optional<BinMatrix> K = A.kernel();
    CHECK(K.has_value() && K->nrows() == 130 && K->ncols() == 90);
    CHECK(A == before);
    CHECK(is_zero(A * *K));
    CHECK(*K == R.stacked(BinMatrix::identity(90)));
  }
  {  // a product of rank at most 100, large enough for the device path of the size dispatch
    BinMatrix A = BinMatrix::random(700, 100) * BinMatrix::random(100, 900), before = A;
    std::optional<BinMatrix> K = A.kernel();
    CHECK(K.has_value() && K->nrows() == 900 && K->ncols() == 900 - A.rank());
    CHECK(A == before);
    CHECK(is_zero(A * *K));
    CHECK(K->rank() == K->ncols());
  }
  CHECK(!BinMatrix::identity(70).kernel().has_value());
  return 0;
}
