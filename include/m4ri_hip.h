/*
 * m4ri_hip.h -- C ABI of libm4ri_hip.so: the MI355X (gfx950) replacement for the part of
 * the M4RI C library that thomwiggers/m4ri-rust reaches on its multiply path.
 *
 * Section 1 is the DROP-IN boundary: the struct layout and the symbols that m4ri-sys declares
 * in `extern "C"` blocks and that the friendly layer (BinMatrix / BinVector) calls.  Every
 * declaration cites the reference interface it replaces (paths relative to the reference
 * repository root).  Host code that links m4ri-sys against this library instead of libm4ri.a
 * needs no source change: see INTEGRATION.md.  (The result side copy, gf2_set_result_side_cols, is
 * opt-in and off by default: it asks the caller to report stores through rows[].)
 *
 * Section 2 is the device-resident API (raw device pointers, explicit HIP stream) used by
 * bench.py, the multi-GPU host layer and callers that chain products without the PCIe round
 * trip.  No torch types appear in any signature.
 *
 * All products are computed on the GPU by hand-written HIP kernels; there is no CPU fallback.
 * If no HIP device is usable the multiply entry points print a diagnostic on stderr and return
 * NULL (the m4ri-rust wrapper turns that into its "Multiplication failed" panic,
 * m4ri-rust/src/friendly/binary_matrix.rs:467-469).
 */
#ifndef M4RI_HIP_H
#define M4RI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ===================================================================================== */
/* 1. M4RI-compatible boundary                                                            */
/* ===================================================================================== */

/* m4ri-sys/src/misc.rs:5-26 */
typedef int rci_t;     /* Rci  */
typedef int wi_t;      /* Wi   */
typedef int BIT;       /* BIT  */
typedef uint64_t word; /* Word */
#define m4ri_radix 64
#define m4ri_one ((word)1)
#define m4ri_ffff ((word)0xffffffffffffffffULL)

/* m4ri-sys/src/mzd.rs:16-21 (MzdBlock) */
typedef struct {
  size_t size; /* bytes in this block */
  word *begin;
  word *end;
} mzd_block_t;

/* m4ri-sys/src/mzd.rs:24-79 (#[repr(C)] Mzd, 64 bytes, size asserted mzd.rs:385).
 * Rust reads nrows/ncols/rows directly (binary_matrix.rs:138,176,286,294) and the private
 * fields in mzd_row / mzd_first_row (mzd.rs:277-313): offsets must not move. */
typedef struct mzd_t {
  rci_t nrows;           /*  0 */
  rci_t ncols;           /*  4 */
  wi_t width;            /*  8  ceil(ncols / 64) */
  wi_t rowstride;        /* 12  words between rows (even-padded when width >= 3) */
  wi_t offset_vector;    /* 16  words from blocks[0].begin to row 0 */
  wi_t row_offset;       /* 20 */
  uint8_t flags;         /* 24  mzd.rs:82-94 */
  uint8_t blockrows_log; /* 25 */
  uint8_t padding[14];   /* 26  (byte 26 holds this library's allocation kind) */
  word high_bitmask;     /* 40  valid bits of the last word of a row */
  mzd_block_t *blocks;   /* 48 */
  word **rows;           /* 56  rows[i] = first word of row i, always a HOST pointer */
} mzd_t;

/* m4ri-sys/src/mzd.rs:82-94 */
#define mzd_flag_nonzero_excess 0x2
#define mzd_flag_windowed_zerooffset 0x4
#define mzd_flag_windowed_zeroexcess 0x8
#define mzd_flag_windowed_ownsblocks 0x10
#define mzd_flag_multiple_blocks 0x20

/* --- container support (host side) --- */
mzd_t *mzd_init(rci_t rows, rci_t cols);                           /* mzd.rs:98  */
void mzd_free(mzd_t *A);                                           /* mzd.rs:102 */
mzd_t *mzd_init_window(mzd_t *M, rci_t lowr, rci_t lowc, rci_t highr, rci_t highc); /* mzd.rs:121-127 */
mzd_t *mzd_copy(mzd_t *dst, mzd_t const *src);                     /* mzd.rs:192 */
int mzd_equal(mzd_t const *A, mzd_t const *B);                     /* mzd.rs:187 */
void mzd_randomize(mzd_t *A);                                      /* mzd.rs:184 */
void mzd_set_ui(mzd_t *A, unsigned int value);                     /* mzd.rs:198 */
mzd_t *mzd_transpose(mzd_t *dst, mzd_t const *A);                  /* mzd.rs:148 */
mzd_t *mzd_add(mzd_t *C, mzd_t const *A, mzd_t const *B);          /* mzd.rs:223 */
mzd_t *mzd_sub(mzd_t *C, mzd_t const *A, mzd_t const *B);          /* mzd.rs:230 */
mzd_t *mzd_concat(mzd_t *C, mzd_t const *A, mzd_t const *B);       /* mzd.rs:195 */
mzd_t *mzd_stack(mzd_t *C, mzd_t const *A, mzd_t const *B);        /* mzd.rs:201 */
mzd_t *mzd_submatrix(mzd_t *S, mzd_t const *M, rci_t lowr, rci_t lowc, rci_t highr, rci_t highc); /* mzd.rs:205-212 */
int mzd_is_zero(mzd_t const *A);                                   /* mzd.rs:233 */
void mzd_row_swap(mzd_t *M, rci_t rowa, rci_t rowb);               /* mzd.rs:130 */
void mzd_copy_row(mzd_t *B, rci_t i, mzd_t const *A, rci_t j);     /* mzd.rs:141 */
void mzd_col_swap(mzd_t *M, rci_t cola, rci_t colb);               /* mzd.rs:144 */
void mzd_row_clear_offset(mzd_t *M, rci_t row, rci_t coloffset);   /* mzd.rs:235-240 */
/* inverse of A by elimination of [A | identity] (identity NULL: built here; inv NULL: allocated); NULL if A is singular. mzd.rs:214-218 */
mzd_t *mzd_invert_naive(mzd_t *inv, mzd_t const *A, mzd_t const *identity);
int m4ri_opt_k(int a, int b, int c);                               /* graycode.rs:56 */
/* T[L[v]] = XOR of the rows r + j of M with bit j of v set, for every k-bit v; Gray-code order; host. brilliantrussian.rs:8-17 */
void mzd_make_table(mzd_t const *M, rci_t r, rci_t c, int k, mzd_t *T, rci_t *L);

/* --- the hot path: every product below runs on the GPU --- */

/* C = A*B, Method of the Four Russians. C may be NULL (allocated). k is M4RI's table-size
 * hint (0 = automatic); the device kernel uses 8-bit tables in LDS whatever k says.
 * brilliantrussian.rs:210-216; caller binary_matrix.rs:59 */
mzd_t *mzd_mul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k);
/* C ^= A*B. brilliantrussian.rs:218-224 */
mzd_t *mzd_addmul_m4rm(mzd_t *C, mzd_t const *A, mzd_t const *B, int k);
/* C = A*B, Strassen recursion over M4RM leaves; cutoff = minimal dimension for recursion,
 * 0 = library default. strassen.rs:8-18; caller binary_matrix.rs:72 (the default `*`) */
mzd_t *mzd_mul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
/* C ^= A*B. strassen.rs:20-31 */
mzd_t *mzd_addmul(mzd_t *C, mzd_t const *A, mzd_t const *B, int cutoff);
/* C = A*B, "naive" entry. mzd.rs:150-152; callers binary_matrix.rs:82 and :427 (mul_slice) */
mzd_t *mzd_mul_naive(mzd_t *C, mzd_t const *A, mzd_t const *B);
/* C ^= A*B. mzd.rs:170-173 */
mzd_t *mzd_addmul_naive(mzd_t *C, mzd_t const *A, mzd_t const *B);
/* C (+)= A * Bt^T with Bt pre-transposed (n x l); clear != 0 overwrites. mzd.rs:154-168 */
mzd_t *_mzd_mul_naive(mzd_t *C, mzd_t const *A, mzd_t const *Bt, int clear);
/* C (+)= v*A, v a 1 x l row. mzd.rs:175-181 */
mzd_t *_mzd_mul_va(mzd_t *C, mzd_t const *v, mzd_t const *A, int clear);

/* -- elimination: blocked Gauss-Jordan on the device, trailing updates through the
 *    multiply kernel.  Each call uploads the matrix, works device-resident, and downloads the result. -- */
/* (Reduced) row echelon form in place; full != 0 -> reduced form (unique), full == 0 -> an upper echelon form with
 * the same pivot columns and row space (row contents then depend on the algorithm, as between M4RI's own variants).
 * Returns the rank.  echelonform.rs:9-16; caller binary_matrix.rs:258-261 (BinMatrix::echelonize, rank :250-252) */
rci_t mzd_echelonize(mzd_t *A, int full);
/* same contract; k (table size of the CPU algorithm) is accepted and ignored. echelonform.rs:29-37 */
rci_t mzd_echelonize_m4ri(mzd_t *A, int full, int k);
/* same contract. echelonform.rs:18-27 */
rci_t mzd_echelonize_pluq(mzd_t *A, int full);
/* dst = src^-1 (dst NULL -> allocated); NULL if src is singular. brilliantrussian.rs:201-208; caller binary_matrix.rs:265-268 */
mzd_t *mzd_inv_m4ri(mzd_t *dst, mzd_t const *src, int k);
/* Solve A X = B.  A is m x n, B has >= max(m, n) rows and holds the right-hand side in its first m rows; on return its
 * first n rows hold X (free variables 0) and the remaining rows are 0; A is overwritten (by its reduced echelon form).
 * Returns 0, or -1 if inconsistency_check != 0 and the system has no solution. solve.rs:12-29; caller binary_matrix.rs:582-586 */
int mzd_solve_left(mzd_t *A, mzd_t *B, int cutoff, int inconsistency_check);

/* --- permutations and PLE / PLUQ (INTEGRATION.md section 3 states the contract) --- */
/* m4ri-sys/src/mzp.rs:10-12 (opaque there): LAPACK-style transposition list, values[i] >= i */
typedef struct mzp_t {
  rci_t *values;
  rci_t length;
} mzp_t;
mzp_t *mzp_init(rci_t length);                                      /* identity; mzp.rs:18 */
void mzp_free(mzp_t *P);                                            /* mzp.rs:21 */
mzp_t *mzp_init_window(mzp_t *P, rci_t begin, rci_t end);           /* values point into P's; mzp.rs:24-27 */
void mzp_free_window(mzp_t *condemned);                             /* frees the window only */
void Mzp_free_window(mzp_t *condemned);                             /* the spelling mzp.rs:29 declares */
mzp_t *mzp_copy(mzp_t *P, mzp_t const *Q);                          /* P NULL: allocated; mzp.rs:32 */
void mzp_set_ui(mzp_t *P, unsigned int value);                      /* 1: identity; anything else aborts; mzp.rs:35 */
void mzp_print(mzp_t const *P);                                     /* one line of values; mzp.rs:38 */
void mzd_apply_p_left(mzd_t *A, mzp_t const *P);                    /* swap rows i, P[i], i ascending; mzp.rs:41 */
void mzd_apply_p_left_trans(mzd_t *A, mzp_t const *P);              /* the same, i descending; mzp.rs:44 */
void mzd_apply_p_right(mzd_t *A, mzp_t const *P);                   /* swap columns i, P[i], i descending; mzp.rs:47 */
void mzd_apply_p_right_trans(mzd_t *A, mzp_t const *P);             /* the same, i ascending; mzp.rs:50 */
/* In place: L below the diagonal, E (mzd_ple) or U (mzd_pluq) from the diagonal on; returns the rank.  P->length must be
 * A->nrows, Q->length A->ncols; cutoff is ignored.  The pivot rows are the row rank profile.  ple.rs:35, ple.rs:65 */
rci_t mzd_ple(mzd_t *A, mzp_t *P, mzp_t *Q, int cutoff);
rci_t mzd_pluq(mzd_t *A, mzp_t *P, mzp_t *Q, int cutoff);
/* solves A0 X = B with A as mzd_pluq left it (free variables 0; B as mzd_solve_left leaves it); -1 only for an inconsistent
 * system with check != 0.  solve.rs:53 */
int mzd_pluq_solve_left(mzd_t const *A, rci_t rank, mzp_t const *P, mzp_t const *Q, mzd_t *B, int cutoff, int check);

/* --- triangular solves (M4RI triangular.h; not declared by m4ri-sys: INTEGRATION.md gives the extern block) ---
 * T is square and unit triangular: only its strict lower (upper) triangle is read, the diagonal counts as 1, and the other
 * triangle and the diagonal may hold anything -- a window of the first r rows and columns of what mzd_pluq leaves serves as L
 * and as U.  X replaces B; it is unique, so every bit is defined, and the device path and the host routine of the size
 * dispatch agree bit for bit.  T and B may be windows, also of one parent, as long as their regions do not overlap; bits of a
 * parent outside B's window do not change.  cutoff (recursion cutoff of the CPU algorithm) is accepted and ignored.  A
 * non-square T or a dimension mismatch aborts, as m4ri_die does; so does a device failure.  n = 0 or an empty B: nothing to do. */
void mzd_trsm_lower_left (mzd_t const *L, mzd_t *B, int cutoff);  /* L X = B,  L n x n, B n x k; X in place of B */
void mzd_trsm_upper_left (mzd_t const *U, mzd_t *B, int cutoff);  /* U X = B */
void mzd_trsm_lower_right(mzd_t const *L, mzd_t *B, int cutoff);  /* X L = B,  B k x n */
void mzd_trsm_upper_right(mzd_t const *U, mzd_t *B, int cutoff);  /* X U = B */

/* --- null space (M4RI solve.h; not declared by m4ri-sys: INTEGRATION.md gives the extern line) ---
 * Returns K (n x (n - r), released with mzd_free) with A K = 0 for the m x n matrix A of rank r, or NULL when r == n or n == 0.  A
 * is overwritten and left holding its reduced row echelon form E, as by mzd_solve_left; it may be a window (bits of the parent
 * outside it do not change).  Every bit of K is defined: with the pivot columns p_0 < ... < p_{r-1} and the free columns f_0 < ... <
 * f_{n-r-1}, row f_j of K is the unit vector e_j and row p_i holds E[i][f_j] in column j.  The order (ascending free columns) is this
 * library's own, not the one M4RI's PLUQ recipe induces; M4RI promises only "an n x (n - r) matrix with A K = 0".  The basis comes
 * from the reduced echelon form, not from a PLUQ factorisation; cutoff is accepted and ignored.  A device failure aborts. */
mzd_t *mzd_kernel_left_pluq(mzd_t *A, int cutoff);

/* ===================================================================================== */
/* 2. Device-resident API                                                                 */
/* ===================================================================================== */

/* A dense bit matrix in device memory: row-major 64-bit words, LSB-first, `ld` words between
 * rows (ld even, base 16-byte aligned), excess bits of the last word zero.  Entries that say "accepts 8-byte-aligned rows" also take
 * views with an odd `ld` or a base at an odd word; the elimination-family entries (echelonize, inverse, ple, apply_p, trsm, solve,
 * nullspace) keep the rule in the parentheses.  tests/test_gpu_mul_views.py holds gf2_mul_dev, gf2_mul_nt_dev and gf2_transpose_dev to
 * it: every route on such views of buffers full of random bits, bit for bit, the words around the views included.
 * Two size limits lie above the shapes callers usually have; both are tested past them, bit for bit (tests/test_gpu_limits.py):
 *  - more than 65 536 x 64 = 4 194 304 rows or columns: gf2_transpose_dev, mzd_transpose, gf2_mul_nt_dev and the products that
 *    transpose B put one workgroup per 64 rows into the y dimension of a launch.  The HIP runtime accepts gridDim.y = 65 538 on this
 *    part (measured: 4 194 369 rows), and so do the row-parallel products, the elimination and gf2_solve_left_dev;
 *  - operands larger than 4 GiB (tested: 9 000 001 x 4096 and 36 929 x 1 048 640): every entry of this section addresses rows with
 *    64-bit offsets.  The tile kernel alone carries 32-bit byte counts: gf2_mul_dev does not make its packed copy of an A of 4 GiB and
 *    more (it reads A in place), and returns -1 with "row stride too large for the tile kernel" for rows of more than about 8 million
 *    columns instead of launching.  nrows and ncols are ints: a dimension stays below 2^31. */
typedef struct {
  uint64_t *data; /* device pointer */
  int64_t ld;     /* words per row stride */
  int nrows;
  int ncols;
} gf2_dmat;

enum { GF2_ALGO_AUTO = 0, GF2_ALGO_M4RM = 1, GF2_ALGO_STRASSEN = 2, GF2_ALGO_NAIVE = 3 };

/* 0 on success, HIP error code (>0) or -1 (bad arguments) otherwise. */
int gf2_device_count(void);                 /* usable HIP devices (0 if none) */
const char *gf2_last_error(void);           /* thread-local text of the last failure */

/* allocation helpers (pooled hipMalloc on the current device).  gf2_dmat_free has hipFree's semantics: it waits for the
 * owning device (the API above is asynchronous; queued work may still use the block) before the block is recycled.
 * gf2_dmat_free_async recycles the block once everything queued on `stream` SO FAR has completed: for matrices that were
 * only used on that one stream (temporaries of a chain of products). */
int gf2_dmat_alloc(gf2_dmat *M, int nrows, int ncols);
void gf2_dmat_free(gf2_dmat *M);
int gf2_dmat_free_async(gf2_dmat *M, void *stream);
int gf2_dmat_upload(gf2_dmat *dst, mzd_t const *src, void *stream);   /* host mzd_t -> device; returns after the copy */
int gf2_dmat_download(mzd_t *dst, gf2_dmat const *src, void *stream); /* device -> host mzd_t */
int gf2_dmat_fill_random(gf2_dmat *M, uint64_t seed, void *stream);   /* splitmix64 stream, same as the oracle */
/* same stream, but M holds rows [row0, row0 + M->nrows) of the full matrix (row-block shards) */
int gf2_dmat_fill_random_rows(gf2_dmat *M, uint64_t seed, int64_t row0, void *stream);
/* general block: rows [row0, ..) x words [col_word0, ..) of a seeded matrix with full_ncols columns (column-panel shards) */
int gf2_dmat_fill_random_block(gf2_dmat *M, uint64_t seed, int64_t row0, int64_t col_word0, int full_ncols, void *stream);

/* --- Arguments and aliasing of the entries below (gf2_mul_dev ... gf2_nullspace_dev) ---
 * Every argument is checked before a device is required and before the first HIP call, so a bad call fails the same way with and
 * without a device: a null struct pointer, a null `data` on a non-empty matrix, a null required out-pointer (`equal`, `singular`,
 * `rank`, `inconsistent`), a negative dimension, an `ld` below the row width, a `data` that is not 8-byte aligned and a shape
 * mismatch return -1 and set gf2_last_error to a text that starts with the entry's name; nothing is launched, allocated or written.
 * Empty shapes return 0 without a launch and without needing a device.  The aliasing check comes last.
 *
 * THE RULE: a matrix that a call writes may share no word with any other matrix argument of that call, except where listed below.
 * Matrices that are only read may be one matrix or overlap freely.  A call that breaks the rule returns -1 ("overlap" in
 * gf2_last_error) before anything is launched.  "Share a word" is decided as for the block calls further down, on whole words: with
 * equal `ld` the two word rectangles are compared exactly, so two column ranges of one parent are fine; with different `ld` any
 * intersection of the address ranges counts.
 *
 * | entry | allowed aliasing | refused (-1, "overlap") |
 * |---|---|---|
 * | `gf2_mul_dev`, `gf2_mul_nt_dev` | A is B / Bt; A and B overlapping; C, A, B three disjoint column ranges of one parent | C sharing a word with A or B (with or without `accumulate`) |
 * | `gf2_add_dev` | C identical to A, to B, or to both (same `data`, `ld`, shape); A is B | C sharing a word with A or B in any other way (shifted by a row, a word, another `ld`) |
 * | `gf2_transpose_dev` | D and S disjoint column ranges of one parent | D sharing a word with S, the square "in place" case included |
 * | `gf2_equal_dev` | anything; A is B gives `*equal = 1` | – |
 * | `gf2_inverse_dev` | Ainv identical to A, or overlapping it in any way (A is copied out before Ainv is written; say so) | – |
 * | `gf2_trsm_dev` | – | B sharing a word with T |
 * | `gf2_solve_left_dev`, `gf2_pluq_solve_left_dev` | – | B sharing a word with A |
 *
 * gf2_inverse_batch_dev keeps its own, stricter rule (stated at its declaration); gf2_copy_block_dev, gf2_submatrix_dev, gf2_concat_dev
 * and gf2_stack_dev state theirs in the paragraph above them; gf2_nullspace_dev allocates K itself, so K cannot alias A. */

/* C (+)= A*B on `stream` (hipStream_t, NULL = default stream); asynchronous.
 * algo: GF2_ALGO_*; param: Strassen levels when algo==STRASSEN (0 = automatic), else ignored.  An explicit level count is honoured as
 * given (at most 6, and as far as the arena fits into device memory): M4RI_HIP_STRASSEN_MAX_LEVELS and M4RI_HIP_STRASSEN_LEAF_MIN
 * bound the automatic choice only.
 * Aliasing: A and B are only read -- A may be B (squaring) and the two may overlap; C is stored tile by tile while other workgroups
 * still read those rows of A and B, so C may share no word with either, with or without `accumulate` (-1, "overlap").  C, A and B may
 * be three disjoint column ranges of one parent.  Accepts 8-byte-aligned rows (tests/test_gpu_mul_views.py): the Strassen passes work
 * on the caller's buffers only when every `ld` is even and every base 16-byte aligned; a product with an odd `ld` or a base at an odd
 * word takes the plain path instead, or, from 1024 rows on, may run its levels on zero-padded copies.
 * An empty C returns 0; an inner dimension of 0 clears C (accumulate: leaves it). */
int gf2_mul_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, int accumulate, int algo, int param,
                void *stream);
/* C (+)= A * Bt^T (row-parity form, mzd.rs:154-168).  Aliasing as gf2_mul_dev: A may be Bt (the Gram matrix A A^T) or overlap it; C
 * may share no word with A or Bt.  Accepts 8-byte-aligned rows (tests/test_gpu_mul_views.py). */
int gf2_mul_nt_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *Bt, int accumulate, void *stream);
/* C = A xor B (mzd.rs:223).  Aliasing: C may be identical to A, to B, or to both (same `data`, `ld` and shape: mzd_add(A, A, B), the
 * reference's +=; every word is read and written by the one thread that owns it), and A may be B (the result is zero).  A C that shares
 * a word with A or B in any other way -- shifted by a row or a word, the same base under another `ld` -- returns -1 ("overlap").
 * Accepts 8-byte-aligned rows: the kernel uses 16-byte accesses only when all three `ld` are even and all three bases 16-byte aligned,
 * and 8-byte accesses otherwise. */
int gf2_add_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream);
/* D = S^T (mzd.rs:148).  Aliasing: D may share no word with S (-1, "overlap"): there is no in-place transposition, not for a square
 * matrix either; D and S may be disjoint column ranges of one parent.  Accepts 8-byte-aligned rows (both kernels read and write caller
 * memory one 8-byte word at a time; tests/test_gpu_mul_views.py). */
int gf2_transpose_dev(gf2_dmat *D, gf2_dmat const *S, void *stream);
/* equality (mzd.rs:187; *equal = 1/0; different shapes: 0; two empty matrices of one shape: 1 without a launch).  Both matrices are only
 * read, so any aliasing is allowed: A is B gives *equal = 1.  Accepts 8-byte-aligned rows (8-byte reads).  Synchronous. */
int gf2_equal_dev(gf2_dmat const *A, gf2_dmat const *B, int *equal, void *stream);
/* Assembly on the device.  The four calls below move bits between ANY bit offsets; destinations are caller-allocated and may be views in
 * a larger buffer.  Every argument is checked before the first HIP call: a destination of the wrong shape, a rectangle that leaves S or
 * D, a negative argument or a null pointer returns -1 and sets gf2_last_error; an empty rectangle returns 0 without a launch.  S and D
 * may be views of one buffer as long as no bit belongs to both rectangles (two column ranges of one parent): with equal `ld` the
 * rectangles are compared exactly, with different `ld` any intersection of their address ranges is refused; overlapping rectangles
 * return -1 (no in-place shift).  Unlike the calls above, these accept views whose rows are only 8-byte aligned (odd `ld`).
 * Asynchronous on `stream`, like gf2_mul_dev. */
/* D[dr+i][dc+j] (^)= S[sr+i][sc+j], i < nrows, j < ncols: any bit offsets. Only the rectangle's bits of D change. */
int gf2_copy_block_dev(gf2_dmat *D, int dr, int dc, gf2_dmat const *S, int sr, int sc, int nrows, int ncols,
                       int accumulate, void *stream);
/* The three below write D / C as a whole matrix: the excess bits of its last word come out zero whatever it held before (a fresh
 * gf2_dmat_alloc block will do), and a view keeps its neighbours. */
/* mzd_submatrix (mzd.rs:205-212): D = S[lowr:highr, lowc:highc]; D must be (highr-lowr) x (highc-lowc) */
int gf2_submatrix_dev(gf2_dmat *D, gf2_dmat const *S, int lowr, int lowc, int highr, int highc, void *stream);
/* mzd_concat (mzd.rs:195): C = [A | B], equal row counts, C is A.nrows x (A.ncols + B.ncols); C may alias neither A nor B */
int gf2_concat_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream);
/* mzd_stack (mzd.rs:201): C = [A ; B], equal column counts */
int gf2_stack_dev(gf2_dmat *C, gf2_dmat const *A, gf2_dmat const *B, void *stream);

/* In-place echelon form of the first ncols_limit columns (0 = all) of a device matrix; the remaining columns follow
 * the row operations (augmented systems).  *rank receives the rank, pivot_cols (host, may be NULL, >= min(rows, limit)
 * ints) the pivot columns.  Synchronous. */
int gf2_echelonize_dev(gf2_dmat *A, int full, int ncols_limit, int *rank, int *pivot_cols, void *stream);
/* Ainv = A^-1 for square A; *singular = 1 (Ainv untouched) if A has no inverse.  Synchronous.  Aliasing: none refused -- A is copied
 * into scratch [A | pad | I] before anything is written and Ainv is written from that scratch after the elimination, so Ainv may be
 * identical to A (inversion in place; a singular A is then left unchanged) or overlap it in any way. */
int gf2_inverse_dev(gf2_dmat *Ainv, gf2_dmat const *A, int *singular, void *stream);
/* --- batched elimination of small matrices (contract per matrix: INTEGRATION.md section 3) ---
 * A batch is `batch` matrices of equal shape stored one below the other in one gf2_dmat: matrix b is rows [b*m, (b+1)*m), so
 * gf2_concat_dev of two stacks is the stack of [A_b | B_b].  Limits: 1 <= m <= 512 rows and 1 <= ncols <= 1024 columns per matrix;
 * a larger shape returns -1 and says so in gf2_last_error (such callers have gf2_echelonize_dev).  A->nrows % m != 0, a null `data`,
 * ld < ceil(ncols / 64) and a negative m or ncols_limit return -1 as well.  Every argument is checked before a device is required;
 * A->nrows == 0 returns 0 without a launch.  A stack may be a strided view: only the ceil(ncols / 64) words of each row are read and
 * written.  Both calls are one launch on `stream`, asynchronous like gf2_mul_dev: no host synchronisation, no allocation. */
/* every matrix of the stack A is replaced by its echelon form, with the contract of gf2_echelonize_dev(full, ncols_limit).  ranks and
 * pivot_cols are DEVICE arrays, either may be NULL: ranks[b] is the rank of matrix b; pivot_cols[b * P + i], P = min(m, limit), is its
 * i-th pivot column for i < ranks[b] and -1 beyond. */
int gf2_echelonize_batch_dev(gf2_dmat *A, int m, int full, int ncols_limit, int *ranks, int *pivot_cols, void *stream);
/* block b of Ainv = (block b of A)^-1 for the n x n blocks (n <= 512) of the stacks A and Ainv; singular[b] (DEVICE, may be NULL) = 1
 * and block b of Ainv left untouched where there is no inverse.  A is not written.  An Ainv of another shape, or one whose address
 * range meets A's, returns -1. */
int gf2_inverse_batch_dev(gf2_dmat *Ainv, gf2_dmat const *A, int n, int *singular, void *stream);
/* which kernel a batch of this shape runs on, without a device: returns a variant id (>= 0), -1 if the shape is outside
 * the limits (inverse != 0: also when ncols != m); out[0] = threads per workgroup, out[1] = matrices per workgroup, out[2] = LDS
 * bytes per workgroup, out[3] = words per row held (identity included for inverse != 0).  Diagnostic, like gf2_tile_plan. */
int gf2_elim_batch_plan(int m, int ncols, int inverse, long long out[4]);
/* mzd_solve_left's contract on device matrices: A is m x n, B has >= max(m, n) rows and holds the right-hand
 * side in its first m rows; on return A holds its reduced row echelon form, rows 0 .. n-1 of B hold X (free variables 0) and every
 * further row of B is zero; *inconsistent = 1 when check != 0 and the system has no solution (B is then as mzd_solve_left leaves it).
 * A and B may be strided views: bits outside them do not change.  m, n or B.ncols equal to 0: returns 0, nothing is done.  A shape
 * error returns -1 and sets gf2_last_error (the host entry aborts instead).  Synchronous on `stream` (the rank must reach the host)
 * and ordered behind the work pending there.  Aliasing: A and B are both written; B may share no word with A (-1, "overlap"). */
int gf2_solve_left_dev(gf2_dmat *A, gf2_dmat *B, int check, int *inconsistent, void *stream);
/* PLE (pluq = 0) or PLUQ (pluq = 1) of a device matrix in place, the layout of mzd_ple / mzd_pluq; P (nrows ints) and Q (ncols
 * ints) are HOST arrays that receive the transposition lists.  Synchronous. */
int gf2_ple_dev(gf2_dmat *A, int pluq, int *P, int *Q, int *rank, void *stream);
/* mzd_apply_p_left (right 0, trans 0), _left_trans (0, 1), _right (1, 0), _right_trans (1, 1) on a device matrix; P: host
 * transposition list of len entries.  Synchronous. */
int gf2_apply_p_dev(gf2_dmat *A, const int *P, int len, int right, int trans, void *stream);
/* mzd_pluq_solve_left on the device: A as gf2_ple_dev(pluq = 1) left it, P / Q host arrays; B (max(nrows, ncols) rows or more)
 * receives X; *inconsistent = 1 when check != 0 finds the system inconsistent.  Synchronous.  Aliasing: B is rewritten step by step
 * while A is still read; B may share no word with A (-1, "overlap"). */
int gf2_pluq_solve_left_dev(gf2_dmat const *A, int rank, const int *P, const int *Q, gf2_dmat *B, int check, int *inconsistent,
                            void *stream);
/* device-resident: B = T^-1 B (right == 0) or B T^-1 (right != 0); upper selects the triangle.  The contract of mzd_trsm_* above:
 * only the strict triangle of T is read, B's bits alone change (the excess bits of its last word stay zero; a view's neighbours stay
 * as they are).  A non-square T or a dimension mismatch returns -1 and sets gf2_last_error; n = 0 or an empty B returns 0 without a
 * launch.  Asynchronous on `stream`, like gf2_mul_dev: one launch inverts the diagonal blocks, the rest is products.  Aliasing: T and B
 * may be views of one buffer, but B may share no word with T (-1, "overlap"): its blocks are rewritten while later steps read T. */
int gf2_trsm_dev(gf2_dmat const *T, gf2_dmat *B, int upper, int right, void *stream);
/* Null space of a device matrix, the contract of mzd_kernel_left_pluq above: A (may be a strided view) is reduced in place to its
 * reduced row echelon form; *K is filled in by the call: n x (n - rank), allocated with gf2_dmat_alloc and freed by the caller with
 * gf2_dmat_free, the excess bits of its last word zero; nullity 0: K = {NULL, 0, n, 0}, nothing allocated.  rank and pivot_cols as in
 * gf2_echelonize_dev.  Synchronous on `stream` (the rank must reach the host before K can be sized) and ordered behind the work
 * pending there.  Bad arguments return -1 and set gf2_last_error. */
int gf2_nullspace_dev(gf2_dmat *A, gf2_dmat *K, int *rank, int *pivot_cols, void *stream);
/* UNSTABLE diagnostic for tools/nullspace_bench.py, not part of the supported interface (it may change or go without notice):
 * event-measured milliseconds of the assembly launch of this thread's last gf2_nullspace_dev that ran while gf2_prof_enable was on */
double gf2_nullspace_last_assembly_ms(void);

/* Strassen levels a product of this shape would use right now (0 = plain M4RM): the cost model's choice, lowered until the
 * operand arena of that many levels fits into free device memory (without a device: the cost model's choice) */
int gf2_strassen_levels(int m, int l, int n, int algo, int param);
/* How a device product of this shape would run, by the cost model (no device needed): returns the Strassen level count;
 * *kind = 0 the shape as given, 1 zero-padded up to dims[0..2], 2 peeled down to the core dims[0..2] (border strips plain) */
int gf2_mul_plan(int m, int l, int n, int algo, int param, int *kind, int dims[3]);
/* How ONE (batched) tile-kernel launch of `batch` products m x l x n would run, by the cost model (no device needed); `packed`:
 * A is handed over row-group packed.  out[0] = kernel variant (7 / 20: 1024- / 256-row tiles x 2048 columns; 8: 2048 x 1024;
 * 9 / 10 / 11 / 12: 4096 / 2048 / 1024 / 512 rows x 512 columns), out[1] = uniform slices of the inner dimension (variants 7, 8,
 * 20), out[2] = tiles cut into stream-K segments and out[3] = number of segments (variants 9-12), out[4] = bytes of scratch
 * for partial tiles; a batched launch may be cut in two -- out[5] = products in the second launch (0: one launch), out[6] / out[7] /
 * out[8] = its variant, tiles cut and segments; returns the modelled time in seconds.  Diagnostic: tools and tests read the
 * launcher's choice from here. */
double gf2_tile_plan(int m, int l, int n, int batch, int packed, long long out[9]);
/* ... and the plan's row band, if it has one: the rows below the last whole tile row of the launch(es) above run in a launch of
 * their own with a shorter tile.  out[0] = rows of the band (0: none; gf2_tile_plan then describes all rows), out[1] = its variant,
 * out[2] / out[3] = its tiles cut and segments, out[4] = its scratch bytes (gf2_tile_plan's out[4] already covers them). */
void gf2_tile_plan_band(int m, int l, int n, int batch, int packed, long long out[5]);
/* modelled seconds of a device product of this shape with exactly `levels` Strassen levels (0: plain M4RM); -1 if that many
 * levels do not divide the shape.  Diagnostic (tools/levels_sweep.py prints it beside the measured time). */
double gf2_model_time(int m, int l, int n, int levels);
/* bytes the Strassen split / merge passes of a product with that many levels read and write (0 for levels == 0): every pass
 * kernel reads its sources once and writes its destinations once, so this is exact; bench.py prices the passes with it */
double gf2_strassen_pass_bytes(int m, int l, int n, int levels);
/* bytes of scratch a product of this shape needs (Strassen operands, packed copies);
 * the library keeps one cached arena per device and grows it on demand. */
size_t gf2_mul_workspace_bytes(int m, int l, int n, int algo, int param);

/* One process, several devices (north_star: "shard row-blocks of A across the GPUs of one node"): C = A*B on host
 * matrices with the rows of A and C divided among `devices` (ndev ordinals in hipGetDeviceCount's numbering; an ordinal may
 * repeat = several shares on one device).  Every share uploads its rows of A and its own copy of B over its own PCIe
 * link, multiplies and downloads its rows of C; the inner dimension is never split, so there is no reduction.  C NULL:
 * allocated.  Returns C, or NULL on failure.  algo / param as gf2_mul_dev.
 * The drop-in entry points (mzd_mul, mzd_mul_m4rm, mzd_mul_naive, strassen.rs:18 / brilliantrussian.rs:216 / mzd.rs:152) do
 * the same by themselves when asked to: M4RI_HIP_DEVICES = "auto" (more than one device visible and the product large: >= 7e13
 * bit operations, >= 4096 rows per share; ignored when WORLD_SIZE > 1, i.e. inside a torch.distributed job) | "all" | "0,1,...".
 * Unset: the current device only.  A single ordinal pins every host entry point (products, elimination, transpose, operand
 * cache) to that device. */
mzd_t *gf2_mul_multi(mzd_t *C, mzd_t const *A, mzd_t const *B, int algo, int param, const int *devices, int ndev);

/* Operand cache for the drop-in entry points: keep a device copy of the host matrix M until gf2_mzd_uncache(M) or
 * mzd_free(M); mzd_mul* calls whose A or B is M then skip its upload (repeated A*v with a fixed A -- mul_slice,
 * binary_matrix.rs:416-431 -- is otherwise bound by moving A over PCIe on every call).  The caller promises not to
 * change M's bits through the host pointers meanwhile (mzd_write_bit and friends on the Rust side are plain stores the
 * library cannot see); library calls that write M or a window of M (as destination, mzd_echelonize, mzd_solve_left, ...)
 * drop the copy themselves: the cache is keyed by the block that M and its windows share. */
int gf2_mzd_cache_on_device(mzd_t const *M);
void gf2_mzd_uncache(mzd_t const *M);

/* Result side copy (opt-in): a product into a NULL destination with at most `cols` columns (and at least 1 MiB
 * of rows) also keeps its packed transposed form on the host, and mzd_transpose of that product is served from it.  Stores through
 * rows[] are invisible to the library, so a caller that opts in must call gf2_mzd_uncache(C) after storing into such a product;
 * without that, mzd_transpose returns the bits of the product as it was computed.  0 = off: the default, unless the environment
 * sets M4RI_HIP_RESULT_SIDE_COLS.  Returns the previous value; takes effect for products that start after the call. */
int gf2_set_result_side_cols(int cols);

/* Host blocks of at least M4RI_HIP_PIN_MIN_BYTES (1 MiB) are pinned so that uploads and downloads run at the PCIe rate; pinning
 * fresh pages costs about 100 ms per 512 MiB, so freed blocks are pooled (up to M4RI_HIP_PIN_CACHE_BYTES, 8 GiB).  A caller that
 * knows its sizes can fill the pool ahead of time: gf2_mzd_prewarm(r, c, count) creates `count` pinned blocks of the size of an
 * r x c matrix (returns how many it added).  The first mzd_init / mzd_mul(NULL, ...) / mzd_transpose(NULL, ...) of that size is
 * then as fast as the later ones. */
int gf2_mzd_prewarm(rci_t r, rci_t c, int count);

/* give cached device memory (per-stream scratch arenas, block cache) of the current device back to the driver;
 * waits for the device first.  The library otherwise keeps what it allocated: the arena of a 131072^3 product is 141 GiB. */
int gf2_trim(void);

/* Size dispatch of the drop-in entry points.  Products of at most M4RI_HIP_HOST_SMALL_WORK
 * word operations (m * l * ceil(n / 64); default 2^20, 0 = every product goes to the device) and echelon forms of that size
 * are computed on the host by the library's own word-parallel routines: the reference's bench shapes (10 x 10 ... 1000 x 64 x
 * 1000, benches/binary_matrix.rs:30-76) take less time there than one PCIe round trip.  The entry points still require a
 * usable device (no fallback: without one they fail as before).  The routines are exported so that they can be checked
 * against the oracle without a device; gf2_host_small_calls() counts how often they ran. */
int gf2_mul_host_small(mzd_t *C, mzd_t const *A, mzd_t const *B, int accumulate);      /* C (+)= A*B; 0 on success */
int gf2_mul_nt_host_small(mzd_t *C, mzd_t const *A, mzd_t const *Bt, int accumulate);  /* C (+)= A*Bt^T */
int gf2_echelonize_host_small(mzd_t *A, int full);                                      /* in place; returns the rank */
int gf2_ple_host_small(mzd_t *A, int pluq, int *P, int *Q);                              /* in place; returns the rank */
/* host routine of the size dispatch of mzd_trsm_* (work = n * n * ceil(k / 64)), exported for tests without a device; 0 on
 * success, -1 for a non-square T or a dimension mismatch */
int gf2_trsm_host_small(mzd_t const *T, mzd_t *B, int upper, int right);
/* host routine of the size dispatch of mzd_kernel_left_pluq (the work measure and limit of mzd_echelonize), exported for tests without
 * a device: gf2_echelonize_host_small (which counts the run) and a word-parallel assembly.  A is left holding its reduced echelon
 * form; *K receives the basis (mzd_free) or NULL for full column rank.  Returns the rank, -1 for a null argument. */
int gf2_nullspace_host_small(mzd_t *A, mzd_t **K);
long long gf2_host_small_calls(void);

/* compact binary file format for host matrices ("GF2M", version, nrows, ncols, dense little-endian rows);
 * 0 / non-NULL on success.  (the reference only serialises to JSON, binary_matrix.rs:10-35) */
int gf2_mzd_save(const char *path, mzd_t const *M);
mzd_t *gf2_mzd_load(const char *path);

/* kernel timing for bench.py's roofline object: HIP events recorded on the launch stream
 * around every launch of the dominant multiply kernel while enabled. */
void gf2_prof_enable(int on);
/* sums since the last reset: *launches, *ms = total event-measured duration of those launches */
int gf2_prof_read(int *launches, double *ms, int reset);

/* Schedules of a large product on HOST matrices (upload / multiply / download pipelines), as the library's time model plays them
 * through: t_end[i] = modelled seconds of schedule i + 1 in M4RI_HIP_HOST_PLAN's numbering, -1 where a schedule does not apply:
 *   1 row blocks of A and C;  2 / 3 / 4 slabs of the inner dimension (four equal; 1/8 1/8 1/4 1/2; two halves), the last slab in row
 *   blocks;  5 / 6 two row groups, each through four equal slabs / two halves;  7 / 8 / 12 the first row group through slabs that grow
 *   from 1/16 (a short lead-in while B arrives), the second through two halves / four quarters / the whole inner dimension;  9 / 10 the
 *   first group through 1/8 1/8 1/4 1/2 / four equal slabs, the second through two halves;  11 one group through the growing slabs.
 * Returns the number of the schedule mzd_mul takes for this shape (0: not pipelined). */
int gf2_host_plan_model(int m, int l, int n, int algo, int param, double t_end[12]);

/* Launch census: "<count> <mangled kernel name>\n" for every kernel of the library this process has launched so far, written to buf
 * (at most cap - 1 bytes and a terminator); returns the length of the whole text.  With M4RI_HIP_KERNEL_CENSUS_FILE=<path> in the
 * environment the counts are also appended to that file when the library is unloaded (child processes of a test suite).  The GPU
 * suite ends with a test that every kernel the shared object contains has been launched (tests/test_zz_kernel_census.py). */
size_t gf2_kernel_census(char *buf, size_t cap);

/* Where the library's device memory came from so far (scratch, the device copies of host operands, gf2_dmat_alloc): out[0] = requests
 * served from the block cache, out[1] = requests served by a fresh hipMalloc.  Read-only; tests/dirty_pool.py uses it to prove that a
 * call ran on blocks it had filled beforehand. */
void gf2_dev_alloc_counts(long long out[2]);

#ifdef __cplusplus
}
#endif
#endif /* M4RI_HIP_H */
