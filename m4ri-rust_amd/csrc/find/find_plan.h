// find_plan.h -- how the row lookup through a hash table runs, in ONE place: the launchers of gf2_find.hip launch what this says,
// find_host.cpp cuts the scratch by it and gf2_find_rows_plan reports it.  Below the plan: the hash of a row's range words, the slot
// that a hash starts at, the slot behind a slot and the layout of a table entry -- the text that the kernels, the host and the CPU
// tests (tests/find_emu.cpp) share.  Plain arithmetic in constexpr functions, which compile for host and device alike; no HIP.
#pragma once
#include <stdint.h>

// ---- the kernels
// A workgroup has kFindThreads lanes.  Lane form: a lane per row, kFindThreads rows per workgroup.  Wave form: a wave per row, and a
// wave takes kFindWaveRows rows one after the other, so a workgroup adds to *count once for kFindWaveGroupRows rows.
constexpr int kFindThreads = 256;
constexpr int kFindWaves = kFindThreads / 64;
constexpr int kFindWaveRows = 16;
constexpr int kFindWaveGroupRows = kFindWaves * kFindWaveRows;
// the widest range, in words of a row, that a single lane still hashes and compares: 8 words are 512 columns; a range of more words
// runs on the wave form, whose 64 lanes read 64 consecutive words at a time
constexpr int kFindLaneWords = 8;
constexpr int kFindLaunches = 3;                   // fill, build, lookup
constexpr long long kFindFillMaxGroups = 1 << 16;  // of the fill kernel, a slot per lane: it strides beyond that

// ---- the table
// slots: the lowest power of two >= 2 NB, so at least half the slots stay empty and every probe sequence ends.  A slot is an ENTRY of
// 64 bits -- the upper 32 bits of the row's hash (the tag) above the row index -- and a member COUNT of 32 bits, in two arrays.
// kFindEmpty, all ones, is no entry: a row index is below 2^31.  Entries of equal rows have equal tags, so among them a smaller entry
// is a lower row, and a 64-bit minimum keeps the lowest.
constexpr uint64_t kFindEmpty = ~0ull;
constexpr int kFindEntryBytes = 8, kFindCountBytes = 4, kFindSlotBytes = kFindEntryBytes + kFindCountBytes;

constexpr uint64_t find_slots(long long nb) {
  uint64_t s = nb > 0 ? 2 : 0;
  while (s < 2 * (uint64_t)nb) s <<= 1;
  return s;
}

// the words of a row that hold a column of [c0, c1): [first, end); an empty range holds no word: both are 0
constexpr long long find_first_word(long long c0, long long c1) { return c0 < c1 ? c0 >> 6 : 0; }
constexpr long long find_end_word(long long c0, long long c1) { return c0 < c1 ? ((c1 - 1) >> 6) + 1 : 0; }

// ---- hash, slots, entries

// a bijection of 64 bits that spreads every input bit over the whole word (the finaliser of splitmix64)
constexpr uint64_t find_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
// what the masked word at position pos = k - first word of the range gives to the hash of its row: the words of a row are combined by
// XOR, so the lanes of a wave hash their words on their own, and the position goes in before the mix, so a row is no multiset of words
constexpr uint64_t find_word_hash(uint64_t masked, long long pos) { return find_mix(masked + 0x9E3779B97F4A7C15ull * (uint64_t)(pos + 1)); }
// the hash of a row from the XOR of its words' parts (0 for an empty range)
constexpr uint64_t find_finish(uint64_t acc) { return find_mix(acc ^ 0xD6E8FEB86659FD93ull); }

// the slot a row's probe sequence starts at -- the low bits of the hash; slots may be 2^32 -- and the slot behind slot s: the
// sequence is linear and wraps
constexpr uint64_t find_first_slot(uint64_t hash, uint64_t slots) { return hash & (slots - 1); }
constexpr uint64_t find_next_slot(uint64_t s, uint64_t slots) { return (s + 1) & (slots - 1); }

// an entry: the tag above the row
constexpr uint64_t find_entry(uint64_t hash, long long row) { return (hash & 0xFFFFFFFF00000000ull) | (uint64_t)row; }
constexpr uint32_t find_entry_tag(uint64_t entry) { return (uint32_t)(entry >> 32); }
constexpr long long find_entry_row(uint64_t entry) { return (long long)(entry & 0xFFFFFFFFull); }

// ---- the plan
struct FindPlan {
  long long slots;        // 0 for NB == 0; -1: bad shape or range
  long long words;        // words of a row that hold a column of the range
  int wave;               // 0: a lane per row, 1: a wave per row
  int launches;           // kFindLaunches; 0 where NA == 0 or NB == 0 (nothing is launched)
  int build_rows;         // rows of B per workgroup of the build kernel
  int lookup_rows;        // rows of A per workgroup of the lookup kernel
  long long entry_bytes;  // the entries, then the counts
  long long scratch;
};

inline FindPlan find_plan(long long nrows_a, long long nrows_b, long long ncols, long long c0, long long c1) {
  FindPlan p = {-1, 0, 0, 0, 0, 0, 0, 0};
  if (nrows_a < 0 || nrows_a > 0x7FFFFFFFll || nrows_b < 0 || nrows_b > 0x7FFFFFFFll || ncols < 0 || ncols > 0x7FFFFFFFll || c0 < 0 || c0 > c1 ||
      c1 > ncols)
    return p;
  p.slots = (long long)find_slots(nrows_b);
  p.words = find_end_word(c0, c1) - find_first_word(c0, c1);
  p.wave = p.words > kFindLaneWords;
  p.launches = nrows_a > 0 && nrows_b > 0 ? kFindLaunches : 0;
  p.build_rows = p.lookup_rows = p.wave ? kFindWaveGroupRows : kFindThreads;
  p.entry_bytes = kFindEntryBytes * p.slots;
  p.scratch = kFindSlotBytes * p.slots;
  return p;
}
