// near_plan.h -- how the Hamming-distance search runs, in ONE place: the launchers of gf2_near.hip launch what this says, near_host.cpp
// cuts the scratch by it and gf2_near_plan reports it.  Plain host arithmetic, no HIP.
//
// A workgroup owns a block of rows of A and one CHUNK of B: the grid is row blocks x S chunks.  A lane keeps the range's words of
// kNearLaneRows rows of A in registers; the chunk goes through LDS in tiles of kNearTileBytes, read by every lane at the same address.
// S is chosen so that a small A still fills the chip; the scratch is one int64 per (row of A, chunk), whatever the number of pairs.
#pragma once

constexpr int kNearThreads = 256;
constexpr int kNearLaneRows = 2;                               // rows of A per lane: every word of B that is read serves two pairs
constexpr int kNearBlockRows = kNearThreads * kNearLaneRows;   // rows of A per workgroup of the register kernels
constexpr int kNearWideBlockRows = kNearThreads;               // ... of the wide kernels: one row per lane, nothing in registers
constexpr int kNearMaxWords = 16;                              // the widest range the register kernels hold: 1024 columns
constexpr int kNearTileBytes = 16384;                          // the tile of B in LDS: 16 KiB / (8 W) rows of W words
constexpr int kNearWideUnit = 64;                              // the wide kernels have no tile: their chunks are multiples of this
constexpr long long kNearTargetGroups = 2048;                  // workgroups wanted at least: 8 per CU of 256
constexpr long long kNearMaxChunkRows = 1 << 20;               // a row's place inside its chunk fits the low 21 bits of a 32-bit key
constexpr int kNearKeyShift = 21;

struct NearPlan {
  int kernel;            // words per row that the kernel is compiled for: 1, 2, 4, 8, 16; 0: the wide kernel; -1: a bad shape
  int words;             // the words of a row that hold a column of the range
  int block_rows;        // rows of A per workgroup
  int tile_rows;         // rows of B per tile (wide: 0)
  int lds;               // LDS bytes
  long long row_blocks;  // blocks of rows of A
  long long chunks;      // S
  long long chunk_rows;  // rows of B per chunk: a multiple of the tile (wide: of kNearWideUnit), at most kNearMaxChunkRows
  long long scratch;     // bytes: one int64 per (row, chunk), and one behind them for the scan's total
};

// the first word of a row that holds a column of [wc0, wc1), and one past the last; an empty range holds no word: both are 0
constexpr long long near_first_word(long long wc0, long long wc1) { return wc0 < wc1 ? wc0 >> 6 : 0; }
constexpr long long near_end_word(long long wc0, long long wc1) { return wc0 < wc1 ? ((wc1 - 1) >> 6) + 1 : 0; }

// the rows of B that chunk c holds: [near_chunk_begin, near_chunk_end)
constexpr long long near_chunk_begin(long long c, long long chunk_rows) { return c * chunk_rows; }
constexpr long long near_chunk_end(long long c, long long chunk_rows, long long nb) {
  const long long e = (c + 1) * chunk_rows;
  return e < nb ? e : nb;
}

// where the int64 of row i of A and chunk c lies: row-major, so that a scan over the cells runs in the order (ia, ib) of the hits
constexpr long long near_cell(long long i, long long chunks, long long c) { return i * chunks + c; }

inline NearPlan near_plan(long long nrows_a, long long nrows_b, long long ncols, long long wc0, long long wc1) {
  NearPlan p = {-1, 0, 0, 0, 0, 0, 0, 0, 0};
  if (nrows_a < 0 || nrows_b < 0 || ncols < 0 || wc0 < 0 || wc0 > wc1 || wc1 > ncols) return p;
  const long long words = near_end_word(wc0, wc1) - near_first_word(wc0, wc1);
  p.words = (int)words;
  p.kernel = words <= 1 ? 1 : words <= 2 ? 2 : words <= 4 ? 4 : words <= 8 ? 8 : words <= kNearMaxWords ? 16 : 0;
  p.block_rows = p.kernel ? kNearBlockRows : kNearWideBlockRows;
  p.tile_rows = p.kernel ? kNearTileBytes / (8 * p.kernel) : 0;
  p.lds = p.kernel ? kNearTileBytes : 0;
  p.row_blocks = (nrows_a + p.block_rows - 1) / p.block_rows;
  const long long unit = p.kernel ? p.tile_rows : kNearWideUnit;
  const long long wanted = (kNearTargetGroups + (p.row_blocks > 1 ? p.row_blocks : 1) - 1) / (p.row_blocks > 1 ? p.row_blocks : 1);
  long long s = (nrows_b + unit - 1) / unit;  // no chunk below a tile
  if (s > wanted) s = wanted;
  if (s < 1) s = 1;
  long long rows = ((nrows_b + s - 1) / s + unit - 1) / unit * unit;
  if (rows < unit) rows = unit;
  if (rows > kNearMaxChunkRows) rows = kNearMaxChunkRows;  // a multiple of every unit
  p.chunk_rows = rows;
  p.chunks = nrows_b > 0 ? (nrows_b + rows - 1) / rows : 1;
  p.scratch = ((8 * (nrows_a * p.chunks + 1)) + 15) & ~15ll;
  return p;
}
