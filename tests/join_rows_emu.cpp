// join_rows_emu.cpp -- the pair, start and head kernels and the index arithmetic of the scatter of the wide join (gf2_join_rows_*_kernel,
// join_rows_chunk_rows and join_rows_output_row of m4ri-rust_amd/csrc/join_rows/gf2_join_rows.hip, cut out of the shipped file by
// tests/test_join_rows_kernels_cpu.py; join_rows_plan.h, which holds join_rows_find_row and join_rows_chunk_outputs, is plain
// arithmetic and is included as it is) on the CPU, thread by thread, under the host compiler's address and undefined-behaviour
// sanitizers.  Every array is a heap block that ENDS with the operand: a read or write behind it is a report.
//
//   without an argument, the program checks itself:
//     the pairs: every window the plan can cut (one of 1 .. 30 bits, and the two of a 31-bit key), as the first window and as a later
//     one, on three workgroups; then the chain of windows with a stable sort in the place of the passes against one stable sort by
//     the whole key.
//     the starts and heads: classes scattered through a pool; only the words of the lowest rows are written.
//     the offsets: runs of rows without outputs, a single row that owns more than a chunk, totals past 2^32, every capacity of
//     interest: the chunk's outputs, its first row and its stretch, and (row of A, rank) of its outputs against a linear walk.
//   with the name of a case file (na nb cap, then rep[nb], idx[na], mult[na]), it runs the whole chain on it -- pairs, a stable sort
//   for the passes, starts, heads, offsets, chunks -- and prints order, head, count, ia and ib, which the test compares with the
//   numpy yardstick (tests/join_rows_ref.py).
#include "kernel_emu.h"
#include "join_rows_plan.h"  // m4ri-rust_amd/csrc/join_rows, as shipped

namespace {
#include KERNEL_BODY
}

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return -1;           \
  } while (0)

// a heap block of exactly n items
template <typename T>
struct Block {
  T *p;
  size_t n;
  explicit Block(size_t n_) : p(new T[n_ ? n_ : 1]), n(n_) {}
  Block(const std::vector<T> &v) : p(new T[v.size() ? v.size() : 1]), n(v.size()) { std::copy(v.begin(), v.end(), p); }
  ~Block() { delete[] p; }
  Block(const Block &) = delete;
};

static dim3 grid_for(long long n, long long per) { return dim3((unsigned)((n + per - 1) / per)); }

// the grouping as the host enqueues it, a stable sort by the window's key standing in for the passes of the class sort
static void group(const std::vector<int> &rep, int bits, std::vector<int> &order) {
  const long long n = (long long)rep.size();
  order.resize(n);
  if (join_rows_windows(bits) == 0) {
    for (long long i = 0; i < n; ++i) order[i] = (int)i;
    return;
  }
  Block<int> r(rep);
  Block<int2> pairs(n);
  for (int win = 0; win < join_rows_windows(bits); ++win) {
    hipLaunchKernelGGL(gf2_join_rows_pairs_kernel, grid_for(n, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, nullptr, r.p, n,
                       join_rows_window_shift(bits, win), join_rows_window_bits(bits, win), win == 0, pairs.p);
    std::stable_sort(pairs.p, pairs.p + n, [](const int2 &a, const int2 &b) { return (u32)a.x < (u32)b.x; });
  }
  for (long long i = 0; i < n; ++i) order[i] = pairs.p[i].y;
}

static long check_pairs() {
  std::mt19937_64 rng(2041);
  const long long n = 2 * kJoinRowsThreads + 88;  // three workgroups, the last one partly
  long cases = 0;
  for (int bits = 1; bits <= 31; ++bits)
    for (int win = 0; win < join_rows_windows(bits); ++win) {
      const int shift = join_rows_window_shift(bits, win), wb = join_rows_window_bits(bits, win);
      if (wb < 1 || wb > kLf2MaxB || shift + wb > bits || (win == 0 && shift != 0)) FAIL("%d bits: window %d is [%d, %d + %d)", bits, win, shift, shift, wb);
      if (win == join_rows_windows(bits) - 1 && shift + wb != bits) FAIL("%d bits: the windows end at %d", bits, shift + wb);
      std::vector<int> rep(n), perm(n);
      for (long long i = 0; i < n; ++i) {
        rep[i] = (int)(rng() & ((1ull << bits) - 1));
        perm[i] = (int)i;
      }
      rep[0] = (int)((1ull << bits) - 1);  // every bit of the key set: bit 30 too
      std::shuffle(perm.begin(), perm.end(), rng);
      for (int first = 0; first < 2; ++first) {
        Block<int> r(rep);
        Block<int2> pairs(n);
        for (long long i = 0; i < n; ++i) pairs.p[i] = make_int2(0x5EAD, perm[i]);
        hipLaunchKernelGGL(gf2_join_rows_pairs_kernel, grid_for(n, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, nullptr, r.p, n, shift, wb, first,
                           pairs.p);
        for (long long i = 0; i < n; ++i) {
          const int row = first ? (int)i : perm[i];
          const u32 want = (u32)(((u64)(u32)rep[row] >> shift) & ((1ull << wb) - 1));
          if (pairs.p[i].y != row || (u32)pairs.p[i].x != want) FAIL("%d bits, window %d, first %d: pair %lld", bits, win, first, i);
        }
        ++cases;
      }
    }
  // the chain of windows is one stable sort by the whole key
  for (int bits : {0, 1, 8, 9, 24, 30, 31}) {
    std::vector<int> rep(n), order, want(n);
    for (long long i = 0; i < n; ++i) {
      rep[i] = bits ? (int)(rng() & ((1ull << bits) - 1)) : 0;
      if (i % 3 == 0 && i) rep[i] = rep[i / 2];  // ties
      want[i] = (int)i;
    }
    std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return (u32)rep[a] < (u32)rep[b]; });
    group(rep, bits, order);
    if (order != want) FAIL("%d bits: the chain of windows does not sort", bits);
    ++cases;
  }
  return cases;
}

// rep of a pool with classes scattered through it: row i belongs to the class of the lowest row with its id
static std::vector<int> random_rep(long long n, int ids, std::mt19937_64 &rng) {
  std::vector<int> id(n), first(ids, -1), rep(n);
  for (long long i = 0; i < n; ++i) {
    id[i] = (int)(rng() % ids);
    if (first[id[i]] < 0) first[id[i]] = (int)i;
    rep[i] = first[id[i]];
  }
  return rep;
}

static int starts_and_heads(const std::vector<int> &rep, const std::vector<int> &order, std::vector<int> &start, std::vector<int> &head) {
  const long long n = (long long)rep.size();
  Block<int> r(rep), o(order), st(n), hd(n);
  for (long long i = 0; i < n; ++i) st.p[i] = hd.p[i] = -77;
  hipLaunchKernelGGL(gf2_join_rows_starts_kernel, grid_for(n, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, nullptr, o.p, r.p, n, st.p);
  for (long long i = 0; i < n; ++i)
    if ((rep[i] == i) != (st.p[i] != -77)) return -1;  // one word per class, at its lowest row, and no other
  hipLaunchKernelGGL(gf2_join_rows_heads_kernel, grid_for(n, kJoinRowsThreads), dim3(kJoinRowsThreads), 0, nullptr, o.p, r.p, st.p, n, hd.p);
  start.assign(st.p, st.p + n);
  head.assign(hd.p, hd.p + n);
  return 0;
}

static long check_starts() {
  std::mt19937_64 rng(2042);
  long cases = 0;
  for (long long n : {1ll, 2ll, 255ll, 256ll, 257ll, 1000ll})
    for (int ids : {1, 3, 100, 5000}) {
      const std::vector<int> rep = random_rep(n, ids, rng);
      std::vector<int> order, start, head;
      group(rep, join_rows_index_bits(n), order);
      if (starts_and_heads(rep, order, start, head)) FAIL("%lld rows, %d ids: a start that is no lowest row, or one missing", n, ids);
      for (long long s = 0; s < n; ++s) {
        const int row = order[s], r = rep[row];
        if (s > 0 && !(rep[order[s - 1]] < r || (rep[order[s - 1]] == r && order[s - 1] < row))) FAIL("%lld rows: the order at %lld", n, s);
        if (order[start[r]] != r || head[s] != start[r] || (start[r] > 0 && rep[order[start[r] - 1]] == r)) FAIL("%lld rows: the head at %lld", n, s);
      }
      ++cases;
    }
  return cases;
}

// the offsets of `mult`, its total, and for a capacity the chunks: everything the scatter computes, against a linear walk
static long check_offsets_of(const std::vector<long long> &mult, long long cap, long long max_chunks) {
  const long long na = (long long)mult.size();
  std::vector<long long> offs(na);
  long long count = 0;
  for (long long i = 0; i < na; ++i) {
    offs[i] = count;
    count += mult[i];
  }
  const Block<long long> o(offs);
  const long long limit = count < cap ? count : cap, chunks = (cap + kJoinRowsChunk - 1) / kJoinRowsChunk;
  long long row = 0, seen = 0;  // the linear walk: `row` owns output t
  long checked = 0;
  for (long long c = 0; c < chunks; ++c) {
    if (max_chunks && c >= max_chunks && c < chunks - max_chunks) continue;  // the first and the last chunks of a giant grid
    long long t0, t1, i0, len;
    const bool any = join_rows_chunk_outputs(c, limit, &t0, &t1);
    if (any != (c * kJoinRowsChunk < limit)) FAIL("chunk %lld of limit %lld: has outputs?", c, limit);
    if (!any) continue;
    if (t0 != c * kJoinRowsChunk || t1 != std::min(t0 + kJoinRowsChunk, limit)) FAIL("chunk %lld: outputs [%lld, %lld)", c, t0, t1);
    join_rows_chunk_rows(o.p, na, t0, t1, &i0, &len);
    if (t0 < seen) FAIL("chunks out of order");
    for (row = t0 >= offs[row] ? row : 0; !(offs[row] <= t0 && t0 < offs[row] + mult[row]); ++row) {}
    if (i0 != row) FAIL("chunk %lld: first row %lld, not %lld", c, i0, row);
    const long long step = t1 - t0 > 64 && max_chunks ? 37 : 1;
    long long last = row;
    if (i0 < 0 || len < 1 || i0 + len > na) FAIL("chunk %lld: the rows [%lld, %lld + %lld) of %lld", c, i0, i0, len, na);
    const Block<long long> stage(std::vector<long long>(offs.begin() + i0, offs.begin() + i0 + len));  // what the workgroup stages
    for (long long t = t0; t < t1; t += (t + step < t1 || t == t1 - 1) ? step : t1 - 1 - t) {
      while (!(offs[last] <= t && t < offs[last] + mult[last])) ++last;
      long long p1, p2;
      const long long r1 = join_rows_output_row(stage.p, i0, len, t, &p1), r2 = join_rows_output_row(o.p + i0, i0, len, t, &p2);
      if (r1 != last || r2 != last || p1 != t - offs[last] || p2 != p1 || p1 < 0 || p1 >= mult[last]) FAIL("output %lld: row %lld rank %lld, not row %lld", t, r1, p1, last);
      ++checked;
    }
    if (i0 + len - 1 != last) FAIL("chunk %lld: %lld rows from %lld, the last output belongs to %lld", c, len, i0, last);
    seen = t1;
  }
  return checked;
}

static long check_offsets() {
  std::mt19937_64 rng(2043);
  long cases = 0, r;
  // runs of rows without outputs between rows with a few, a stretch longer than a chunk of rows, a row that owns several chunks
  std::vector<long long> mult(9000, 0);
  for (size_t i = 0; i < mult.size(); ++i)
    if (i < 3000 ? rng() % 7 == 0 : i > 6000 && rng() % 2) mult[i] = 1 + (long long)(rng() % 4);
  mult[3000] = 3 * kJoinRowsChunk + 5;
  mult[8999] = 0;
  long long total = 0;
  for (long long m : mult) total += m;
  for (long long cap : {1ll, 2ll, (long long)kJoinRowsChunk, kJoinRowsChunk + 1ll, total - 1, total, total + 1, 4 * total}) {
    if ((r = check_offsets_of(mult, cap, 0)) < 0) return -1;
    cases += r;
  }
  // one row, one output; every row zero but the last
  for (auto v : {std::vector<long long>{1}, std::vector<long long>{0, 0, 0, 7}, std::vector<long long>{5000, 0, 0}, std::vector<long long>{0, 0}}) {
    if ((r = check_offsets_of(v, 10000, 0)) < 0) return -1;
    cases += r;
  }
  // totals past 2^32: 65536 rows of 65536 partners each (exactly 2^32), and a few giant rows between rows without outputs
  std::vector<long long> square(65536, 65536);
  for (long long cap : {1000ll, 0x7FFFFFFFll}) {
    if ((r = check_offsets_of(square, cap, 3)) < 0) return -1;
    cases += r;
  }
  std::vector<long long> giant = {0, 0x7FFFFFFFll, 0, 0, 0x7FFFFFFFll, 3, 0x7FFFFFFFll, 0};
  if ((r = check_offsets_of(giant, 0x7FFFFFFFll, 3)) < 0) return -1;
  cases += r;
  long long sum = 0;
  for (long long m : giant) sum += m;
  if (sum <= (1ll << 32)) FAIL("the giant rows do not pass 2^32");
  return cases;
}

static int run_case(const char *path) {
  FILE *f = fopen(path, "r");
  long long na, nb, cap;
  if (!f || fscanf(f, "%lld %lld %lld", &na, &nb, &cap) != 3) return 2;
  std::vector<int> rep(nb), idx(na), multi(na);
  for (auto *v : {&rep, &idx, &multi})
    for (int &x : *v)
      if (fscanf(f, "%d", &x) != 1) return 2;
  fclose(f);
  std::vector<int> order, start, head;
  group(rep, join_rows_index_bits(nb), order);
  if (starts_and_heads(rep, order, start, head)) return 3;
  std::vector<long long> offs(na);
  long long count = 0;
  for (long long i = 0; i < na; ++i) {
    offs[i] = count;
    count += multi[i];
  }
  printf("order");
  for (int x : order) printf(" %d", x);
  printf("\nhead");
  for (int x : head) printf(" %d", x);
  printf("\ncount %lld\n", count);
  const Block<long long> o(offs);
  const Block<int> ord(order), st(start), ix(idx);
  const long long limit = count < cap ? count : cap;
  std::vector<int> ia, ib;
  for (long long c = 0; c < (cap + kJoinRowsChunk - 1) / kJoinRowsChunk; ++c) {
    long long t0, t1, i0, len, p;
    if (!join_rows_chunk_outputs(c, limit, &t0, &t1)) continue;
    join_rows_chunk_rows(o.p, na, t0, t1, &i0, &len);
    for (long long t = t0; t < t1; ++t) {
      const long long i = join_rows_output_row(o.p + i0, i0, len, t, &p);
      ia.push_back((int)i);
      ib.push_back(ord.p[st.p[ix.p[i]] + p]);
    }
  }
  printf("ia");
  for (int x : ia) printf(" %d", x);
  printf("\nib");
  for (int x : ib) printf(" %d", x);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1) return run_case(argv[1]);
  const long pairs = check_pairs();
  if (pairs < 0) return 1;
  printf("%ld pair cases ok\n", pairs);
  const long starts = check_starts();
  if (starts < 0) return 1;
  printf("%ld start cases ok\n", starts);
  const long outputs = check_offsets();
  if (outputs < 0) return 1;
  printf("%ld outputs ok\n", outputs);
  return 0;
}
