// find_emu.cpp -- the hash, the compare, the slot sequence and the lane forms of insert and probe of the row lookup (find_row_hash,
// find_rows_equal, find_insert and find_probe of m4ri-rust_amd/csrc/find/gf2_find.hip, with gf2_word_mask of gf2_dev_words.h, which
// they use; cut out of the shipped files by tests/test_find_helpers_cpu.py; find_plan.h is plain arithmetic and is included as it is)
// on the CPU, one thread after the other, under the host compiler's address and undefined-behaviour sanitizers.
//   hash and compare: two rows in heap blocks of ONLY the words of the range.  Equal on the range with every bit outside it flipped:
//   one hash, equal.  One column of the range flipped, for every column: another hash (the mix is a bijection and one word changed),
//   different, and the blocks of the compare END with the word of that column -- it may not read on behind the first difference.
//   the slot sequence: from every slot of a table of 2, 4, 8 and 64 slots, `slots` steps visit every slot once and return; 2^32 slots.
//   the table: a serial build and lookup with tables FORCED SMALL -- 4, 8 and 64 slots with slots - 1 distinct rows plus duplicates,
//   loads that the device entry never reaches: chains wrap around the end of the table, a miss ends at the one empty slot, and the
//   lowest row of a class stays whatever order the rows arrive in.  B and A live in heap blocks that begin with the first range word
//   of their first row and end with the last range word of their last row; entries and counts are `slots` long.  The pools and the
//   results are printed; the Python test compares them with tests/find_ref.py.
// A read of any other word is a report of the address sanitizer.
#include "kernel_emu.h"
#include "find_plan.h"  // m4ri-rust_amd/csrc/find, as shipped

typedef unsigned long long FindEntry;
// one thread after the other: an atomic is its plain form
static FindEntry atomicCAS(FindEntry *p, FindEntry expected, FindEntry desired) {
  const FindEntry old = *p;
  if (old == expected) *p = desired;
  return old;
}
static FindEntry atomicMin(FindEntry *p, FindEntry v) {
  const FindEntry old = *p;
  if (v < old) *p = v;
  return old;
}
static u32 atomicAdd(u32 *p, u32 v) {
  const u32 old = *p;
  *p = old + v;
  return old;
}

namespace {
#include KERNEL_BODY
}

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return -1;           \
  } while (0)

// a heap block of the words [w0, w1) of `row` alone, addressed like the row
struct Part {
  u64 *block;
  const u64 *row;
  Part(const std::vector<u64> &full, long long w0, long long w1) {
    block = new u64[w1 - w0];
    for (long long k = w0; k < w1; ++k) block[k - w0] = full[k];
    row = reinterpret_cast<const u64 *>(reinterpret_cast<uintptr_t>(block) - 8 * (uintptr_t)w0);
  }
  ~Part() { delete[] block; }
};

static long check_hash_and_compare(const int *widths, int nwidths) {
  std::mt19937_64 rng(2101);
  long cases = 0;
  for (int t = 0; t < nwidths; ++t) {
    const int ncols = widths[t], nw = (ncols + 63) >> 6;
    std::vector<u64> a(nw);
    for (int k = 0; k < nw; ++k) a[k] = rng();
    for (int c0 = 0; c0 <= ncols; ++c0)
      for (int c1 = c0; c1 <= ncols; ++c1) {
        const long long w0 = find_first_word(c0, c1), w1 = find_end_word(c0, c1);
        if (c0 < c1 && (w0 != (c0 >> 6) || w1 != ((c1 - 1) >> 6) + 1)) FAIL("ncols %d [%d, %d): words [%lld, %lld)", ncols, c0, c1, w0, w1);
        if (c0 == c1 && w0 != w1) FAIL("ncols %d: the empty range [%d, %d) holds a word", ncols, c0, c1);
        std::vector<u64> b(nw);
        for (int k = 0; k < nw; ++k) b[k] = ~a[k];                    // every bit outside the range differs, the excess bits too ...
        for (int c = c0; c < c1; ++c) b[c >> 6] ^= 1ull << (c & 63);  // ... and inside it none
        u64 ha;
        {
          const Part pa(a, w0, w1), pb(b, w0, w1);
          ha = find_row_hash(pa.row, w0, w1, c0, c1);
          if (ha != find_row_hash(pb.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): rows that are equal on the range hash apart", ncols, c0, c1);
          if (!find_rows_equal(pa.row, pb.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): rows that are equal on the range differ", ncols, c0, c1);
          if (!find_rows_equal(pa.row, pa.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): a row differs from itself", ncols, c0, c1);
          if (c0 == c1 && ha != find_finish(0)) FAIL("ncols %d: the hash of the empty range [%d, %d)", ncols, c0, c1);
        }
        ++cases;
        for (int c = c0; c < c1; ++c) {  // one column flipped
          b[c >> 6] ^= 1ull << (c & 63);
          {
            const Part pb(b, w0, w1);
            if (find_row_hash(pb.row, w0, w1, c0, c1) == ha) FAIL("ncols %d [%d, %d): column %d is not hashed", ncols, c0, c1, c);
          }
          const Part pa(a, w0, (c >> 6) + 1), pb(b, w0, (c >> 6) + 1);  // the blocks end with its word
          if (find_rows_equal(pa.row, pb.row, w0, w1, c0, c1)) FAIL("ncols %d [%d, %d): a difference in column %d is not seen", ncols, c0, c1, c);
          b[c >> 6] ^= 1ull << (c & 63);
          ++cases;
        }
      }
  }
  return cases;
}

static long check_slots() {
  long cases = 0;
  for (u64 slots : {2ull, 4ull, 8ull, 64ull}) {
    if (find_slots((long long)(slots / 2)) != slots) FAIL("find_slots(%llu)", (unsigned long long)(slots / 2));
    for (u64 first = 0; first < slots; ++first) {
      std::vector<int> seen(slots, 0);
      u64 s = find_first_slot(first + 0xABCDEF0000000000ull * slots, slots);  // only the low bits choose the slot
      if (s != first) FAIL("%llu slots: the first slot", (unsigned long long)slots);
      for (u64 step = 0; step < slots; ++step, s = find_next_slot(s, slots)) {
        if (s >= slots || seen[s]++) FAIL("%llu slots: slot %llu out of range or twice", (unsigned long long)slots, (unsigned long long)s);
      }
      if (s != first) FAIL("%llu slots: the sequence does not wrap", (unsigned long long)slots);
      ++cases;
    }
  }
  const u64 big = 1ull << 32;
  if (find_slots((1ll << 30) + 1) != big || find_slots(0x7FFFFFFFll) != big || find_slots(0) != 0 || find_slots(1) != 2)
    FAIL("find_slots at the ends");
  if (find_first_slot(0x123456789ABCDEF0ull, big) != 0x9ABCDEF0ull || find_next_slot(big - 1, big) != 0 || find_next_slot(0x7FFFFFFFull, big) != 0x80000000ull)
    FAIL("2^32 slots");
  // an entry: the tag above the row; entries of one tag order by row; none is the empty value
  const u64 h = 0xFFFFFFFF12345678ull;
  if (find_entry_row(find_entry(h, 0x7FFFFFFF)) != 0x7FFFFFFF || find_entry_tag(find_entry(h, 5)) != 0xFFFFFFFFu || find_entry(h, 0x7FFFFFFF) == kFindEmpty ||
      !(find_entry(h, 3) < find_entry(h, 4)))
    FAIL("entries");
  return cases + 3;
}

// rows of ncols bits, ld words apart, in a block that holds nothing before word w0 of row 0 and nothing behind word w1 - 1 of the last
struct Pool {
  u64 *block = nullptr;
  const u64 *base = nullptr;
  Pool(const std::vector<std::vector<u64>> &rows, long long ld, long long w0, long long w1) {
    const long long n = (long long)rows.size();
    if (n == 0) return;
    if (w0 == w1) {  // no word is read (check_hash_and_compare holds that): an address for the row arithmetic
      base = block = new u64[1];
      return;
    }
    const long long len = (n - 1) * ld + (w1 - w0);
    block = new u64[len];
    std::mt19937_64 junk(7);
    for (long long i = 0; i < len; ++i) block[i] = junk();  // the words between the rows are dirty
    for (long long r = 0; r < n; ++r)
      for (long long k = w0; k < w1; ++k) block[r * ld + k - w0] = rows[r][k];
    base = reinterpret_cast<const u64 *>(reinterpret_cast<uintptr_t>(block) - 8 * (uintptr_t)w0);
  }
  ~Pool() { delete[] block; }
};

static void print_rows(const char *tag, const std::vector<std::vector<u64>> &rows) {
  for (const auto &r : rows) {
    printf("%s", tag);
    for (u64 x : r) printf(" %016llx", (unsigned long long)x);
    printf("\n");
  }
}

static long check_tables() {
  std::mt19937_64 rng(2102);
  long cases = 0;
  const int shapes[][3] = {{130, 1, 129}, {200, 57, 200}, {64, 0, 64}, {300, 70, 71}, {100, 40, 40}};  // ncols, c0, c1
  for (u64 slots : {4ull, 8ull, 64ull})
    for (const auto &shape : shapes) {
      const int ncols = shape[0], c0 = shape[1], c1 = shape[2], nw = (ncols + 63) >> 6;
      const long long w0 = find_first_word(c0, c1), w1 = find_end_word(c0, c1), ldb = nw + 3, lda = nw + 1;
      // slots - 1 distinct values of the range (an id in its low bits keeps them apart; one column: two values; none: one)
      const int width = c1 - c0;
      const int distinct = width == 0 ? 1 : width == 1 ? 2 : (int)slots - 1;
      auto value_row = [&](int id, bool fresh) {
        std::vector<u64> row(nw);
        for (auto &x : row) x = rng();  // junk everywhere, the excess bits too
        if (width >= 2) {
          // below the id bits the range is a function of the id; a fresh row carries an id that no row of B has
          std::mt19937_64 of_id(1000 + id);
          for (int c = c0; c < c1; ++c) {
            const u64 bit = of_id() & 1;
            row[c >> 6] = (row[c >> 6] & ~(1ull << (c & 63))) | (bit << (c & 63));
          }
          const int idbits = width < 8 ? width : 8, v = fresh ? id + 128 : id;
          for (int j = 0; j < idbits; ++j) row[(c0 + j) >> 6] = (row[(c0 + j) >> 6] & ~(1ull << ((c0 + j) & 63))) | ((u64)((v >> j) & 1) << ((c0 + j) & 63));
        } else if (width == 1) {
          row[c0 >> 6] = (row[c0 >> 6] & ~(1ull << (c0 & 63))) | ((u64)(id & 1) << (c0 & 63));
        }
        return row;
      };
      std::vector<std::vector<u64>> B, A;
      for (int id = 0; id < distinct; ++id) B.push_back(value_row(id, false));
      for (int d = 0; d < (int)slots / 2 + 1; ++d) B.push_back(value_row((int)(rng() % distinct), false));  // duplicates
      std::shuffle(B.begin(), B.end(), rng);
      const int nb = (int)B.size(), na = 2 * (int)slots + 3;
      for (int i = 0; i < na; ++i) A.push_back(value_row((int)(rng() % distinct), width >= 8 && (i & 1)));
      const Pool pb(B, ldb, w0, w1), pa(A, lda, w0, w1);
      std::vector<int> first_idx, first_mult;
      for (int round = 0; round < 3; ++round) {  // three arrival orders: ascending, descending, shuffled
        std::vector<int> arrival(nb);
        for (int j = 0; j < nb; ++j) arrival[j] = round == 1 ? nb - 1 - j : j;
        if (round == 2) std::shuffle(arrival.begin(), arrival.end(), rng);
        FindEntry *entries = new FindEntry[slots];
        u32 *counts = new u32[slots];
        for (u64 s = 0; s < slots; ++s) entries[s] = kFindEmpty, counts[s] = 0;
        for (int j : arrival) find_insert(pb.base, ldb, j, w0, w1, c0, c1, entries, slots, counts);
        u64 used = 0, members = 0;
        for (u64 s = 0; s < slots; ++s) used += entries[s] != kFindEmpty, members += counts[s];
        if (used != (u64)distinct || members != (u64)nb) FAIL("%llu slots: %llu classes, %llu members", (unsigned long long)slots, (unsigned long long)used, (unsigned long long)members);
        std::vector<int> idx(na), mult(na);
        for (int i = 0; i < na; ++i) {
          idx[i] = find_probe(pa.base + (long long)i * lda, pb.base, ldb, w0, w1, c0, c1, entries, slots, counts, &mult[i]);
          int none = -7;
          if (find_probe(pa.base + (long long)i * lda, pb.base, ldb, w0, w1, c0, c1, entries, slots, nullptr, &none) != idx[i] || none != 0)
            FAIL("a probe without counts");
        }
        delete[] entries;
        delete[] counts;
        if (round == 0) {
          first_idx = idx;
          first_mult = mult;
        } else if (idx != first_idx || mult != first_mult)
          FAIL("%llu slots, ncols %d [%d, %d): the result depends on the arrival order", (unsigned long long)slots, ncols, c0, c1);
      }
      printf("CASE %llu %d %d %d %d %d\n", (unsigned long long)slots, ncols, c0, c1, na, nb);
      print_rows("B", B);
      print_rows("A", A);
      printf("IDX");
      for (int x : first_idx) printf(" %d", x);
      printf("\nMULT");
      for (int x : first_mult) printf(" %d", x);
      printf("\n");
      ++cases;
    }
  return cases;
}

int main() {
  const int widths[] = {1, 63, 64, 65, 130};
  const long compares = check_hash_and_compare(widths, 5);
  if (compares < 0) return 1;
  printf("%ld hashes and compares ok\n", compares);
  const long slots = check_slots();
  if (slots < 0) return 1;
  printf("%ld slot sequences ok\n", slots);
  const long tables = check_tables();
  if (tables < 0) return 1;
  printf("%ld tables ok\n", tables);
  return 0;
}
