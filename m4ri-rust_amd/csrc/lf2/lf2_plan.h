// lf2_plan.h -- how the class sort and an LF2 round run, in ONE place: the launchers of gf2_lf2.hip launch what this says, lf2_host.cpp
// cuts the scratch by it and gf2_lf2_plan reports it (the way bkw_plan.h serves LF1).  Plain host arithmetic, no HIP.
#pragma once

constexpr int kLf2MaxB = 30;  // the key of m4ri_hip_bkw.h: at most two words of a row

// ---- the sort: a least-significant-digit radix sort of (key, row) pairs
// A pass sorts by kLf2DigitBits bits of the key (the last one by what is left).  A workgroup of kLf2Threads lanes owns a tile of
// kLf2TileRows consecutive items; the tiles' digit counts lie digit-major (counts[digit * tiles + tile]), so that their exclusive sums
// in that order are the places where a tile's items of a digit go.  The tile is large so that the counts are few: 2^26 rows give
// 256 * 2^14 counts, scanned in two levels of kLf2ScanChunk counts per workgroup.
constexpr int kLf2DigitBits = 8;
constexpr int kLf2Digits = 1 << kLf2DigitBits;
constexpr int kLf2Threads = 256;
constexpr int kLf2Waves = kLf2Threads / 64;
constexpr int kLf2TileItems = 16;  // items per lane of a sort tile
constexpr int kLf2TileRows = kLf2Threads * kLf2TileItems;
constexpr int kLf2WaveRows = kLf2TileRows / kLf2Waves;  // the consecutive items of a tile that one wave ranks
constexpr int kLf2ScanItems = 8;                        // counts per lane of a scan workgroup
constexpr int kLf2ScanChunk = kLf2Threads * kLf2ScanItems;
constexpr int kLf2SortLds = 4 * kLf2Waves * kLf2Digits;  // bytes: the running counts of the scatter kernel, one row per wave

// ---- the pairs
// A workgroup owns a run of kLf2RunRows consecutive sorted positions, kLf2RunItems consecutive ones per lane.  The scatter deals the
// run's OUTPUTS to groups of `lanes` lanes (1, 2, 8 or 64 by the row width, as the LF1 scatter and the row gather cut it).
constexpr int kLf2RunItems = 4;
constexpr int kLf2RunRows = kLf2Threads * kLf2RunItems;
constexpr int kLf2PieceWords = 2;  // 16 bytes
constexpr int kLf2NarrowWords = 4;
constexpr int kLf2MidWords = 64;

inline long long lf2_align16(long long bytes) { return (bytes + 15) & ~15ll; }

struct Lf2Plan {
  int passes;              // of the sort: ceil(b / 8), 0 for b == 0; -1: bad shape
  int lanes;               // lanes per row of the pair scatter
  long long tiles;         // sort tiles
  long long runs;          // runs of the pair kernels
  long long pair_bytes;    // one buffer of (key, row) pairs
  long long count_bytes;   // the digit counts of one pass
  long long part_bytes;    // the chunk sums of their scan
  long long sort_scratch;  // gf2_class_sort_dev: two pair buffers, counts, chunk sums
  long long order_bytes;   // order (and as much again for skeys) of gf2_lf2_reduce_dev
  long long pair_scratch;  // gf2_lf2_reduce_dev: order, skeys, run sums
};

inline Lf2Plan lf2_plan(long long nrows, long long ncols, int b) {
  if (nrows < 0 || ncols < 0 || b < 0 || b > kLf2MaxB) return {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  Lf2Plan p;
  p.passes = (b + kLf2DigitBits - 1) / kLf2DigitBits;
  const long long nw = (ncols + 63) >> 6;
  p.lanes = nw <= kLf2PieceWords ? 1 : nw <= kLf2NarrowWords ? 2 : nw <= kLf2MidWords ? 8 : 64;
  p.tiles = (nrows + kLf2TileRows - 1) / kLf2TileRows;
  p.runs = (nrows + kLf2RunRows - 1) / kLf2RunRows;
  p.pair_bytes = lf2_align16(8 * nrows);
  p.count_bytes = lf2_align16(4ll * kLf2Digits * p.tiles);
  p.part_bytes = lf2_align16(4 * ((kLf2Digits * p.tiles + kLf2ScanChunk - 1) / kLf2ScanChunk));
  p.sort_scratch = 2 * p.pair_bytes + p.count_bytes + p.part_bytes;
  p.order_bytes = lf2_align16(4 * nrows);
  p.pair_scratch = 2 * p.order_bytes + lf2_align16(8 * p.runs);
  return p;
}

// the sort's work space, sort_scratch bytes from `base` on: two pair buffers, the digit counts, the chunk sums of their scan
struct Lf2SortWork {
  void *pairs[2];
  int *counts, *parts;
};
inline Lf2SortWork lf2_sort_work(void *base, const Lf2Plan &p) {
  char *at = static_cast<char *>(base);
  return {{at, at + p.pair_bytes}, reinterpret_cast<int *>(at + 2 * p.pair_bytes), reinterpret_cast<int *>(at + 2 * p.pair_bytes + p.count_bytes)};
}

// the bits of pass `pass`: [kLf2DigitBits * pass, ...) of the key
inline int lf2_pass_bits(int b, int pass) {
  const int left = b - kLf2DigitBits * pass;
  return left > kLf2DigitBits ? kLf2DigitBits : left;
}
