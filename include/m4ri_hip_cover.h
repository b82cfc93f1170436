/* m4ri_hip_cover.h -- companion of m4ri_hip.h, section 2 (device-resident API): the COVERING-CODE reduction ON THE DEVICE.  Behind a
 * few LF1 rounds (m4ri_hip_bkw.h) the window of sample bits that is left is cut into blocks; every block is decoded to the nearest
 * codeword of a small [n, k] code, the codeword's message bits replace the block, and the label stays.  The samples get shorter at the
 * price of more noise and of NO sample, and the pool that comes out is what gf2_lpn_errors_dev and gf2_min_weight_dev (m4ri_hip_wht.h)
 * score: LF1 rounds, cover, errors, minimum are one chain on the caller's stream.  DESIGN.md section 7.12; INTEGRATION.md sections 3, 4.
 *
 * Every row depends on itself alone, so the result is exact and does not depend on launch order.  Two runs give the same bits.
 *
 * A code is [n, k] with r = n - k check bits, in systematic form: bit t of the syndrome of an n-bit block a is parity(a & h[t]), bit j
 * of a is the block's column j, and the rows must satisfy h[t] >> k == 1u << t, so a codeword is (u, A u) and its message is its low k
 * bits.  Limits: 1 <= n <= 32, 0 <= k <= n, and r <= 12 when 1 <= k < n.  r == 0 is the identity code: the bits pass through.  k == 0
 * is the zero code: the bits are dropped.  Both need neither h nor a table, neither is read for them, and their n may be anything up
 * to 32.
 *
 * gf2_cover_leaders (host, no device).  leaders[s], for every s in [0, 2^r), is the pattern e with syndrome s of LOWEST weight, among
 * patterns of equal weight the one smallest as an integer; *radius (may be NULL) is the largest weight, the covering radius.  It runs
 * in O(2^r n): a leader without its top bit is the leader of its own syndrome, so one pass per weight over the syndromes suffices.  -1
 * for a code that breaks the limits above, for bits of h at or above n and for a non-systematic h.  For k == 0 or r == 0 it writes
 * leaders[0] = 0 when r == 0 and nothing else, and returns 0.
 *
 * gf2_cover_code_named (host, no device); anything else returns -1:
 *     GF2_COVER_IDENTITY(n), GF2_COVER_DROP(n)   1 <= n <= 32; [n, n] and [n, 0]; h is zero
 *     GF2_COVER_REPETITION(n)                    2 <= n <= 13; [n, 1]; h[t] = 1 | 1 << (1 + t)
 *     GF2_COVER_HAMMING(r)                       2 <= r <= 5; [2^r - 1, 2^r - 1 - r]; column j < k of A is the j-th smallest integer of
 *                                                [1, 2^r) that is not a power of two, with bit t of it in h[t]
 *     GF2_COVER_GOLAY23 (param 0)                [23, 12]; column i of A is x^(11+i) mod g, g = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1,
 *                                                bit t the coefficient of x^t; its leaders have the weights 0..3 (1, 23, 253, 1771)
 *
 * gf2_cover_reduce_dev.  Segment j uses code c = seg_code[j].  It reads the block a = bits [o_j, o_j + n_c) of row i of P, where
 * o_j = c0 + the lengths of the segments before it.  With s the syndrome of a, the error pattern e is leaders[c][s] & mask(n) when a
 * table is read, 0 for r == 0, a for k == 0.  It writes (a ^ e) & mask(k) to bits [q_j, q_j + k_c) of row i of D, where q_j = the
 * dimensions of the segments before it, and dist[i] = the sum over j of popcount(e) (dist may be NULL).  D->ncols must equal K = the
 * sum of k, D->nrows must equal P->nrows, and the window [c0, c0 + sum of n) must lie inside P; columns outside it are ignored.  The
 * tables are taken as they are: a table that is no leader table still has the result the formulas say.  leaders is a HOST array of
 * ncodes DEVICE pointers (2^r words each); the entry of a code without a table, or of a code that no segment uses, is not read.
 *
 * What is written.  D's rows are written as whole rows by the rule of gf2_submatrix_dev: the excess bits of the last word are zero, and
 * a view keeps its neighbouring words.  D and dist are OVERWRITTEN: the caller zeroes nothing.
 *
 * What is read.  Only the window bits of P are read: a word of a row is read only when it holds a bit of the window.  Pad words and
 * excess bits are never read, so P may be a strided view of a dirty parent.  Nothing of P is written.  A block spans at most two words.
 * Rows that are only 8-byte aligned (an odd `ld`, a base on an odd word) are accepted; 16-byte accesses are used only where every row
 * of P, and independently of D, starts on a 16-byte boundary.  Rows are addressed with 64-bit offsets, so operands past 4 GiB work.
 *
 * Asynchronous on `stream`, like gf2_mul_dev: no host synchronisation, no hipMalloc and no scratch.  Codes and segment indices travel
 * as kernel arguments, the tables are the caller's and are copied into LDS once per workgroup.
 *
 * Degenerate shapes.  With nrows == 0 nothing is launched.  With nseg == 0 or K == 0, D has no column and only dist is written.
 *
 * Arguments are checked before a device is required and before the first HIP call; -1, and gf2_last_error starts with the entry's
 * name: a null P or D, a null `data` on a non-empty matrix, a negative dimension, an `ld` below the row width, a `data` that is not
 * 8-byte aligned, a dist or a table that is not 4-byte aligned, ncodes outside 1..16 (0 is accepted with nseg == 0), nseg outside
 * 0..256, a null codes, seg_code or leaders that would be read, a seg_code[j] >= ncodes, a bad code (the rules of gf2_cover_leaders),
 * a null table of a code that needs one and that a segment uses, more than GF2_COVER_MAX_LEADERS table words (the sum of 2^r over the
 * codes that have a table), a window outside P, D->ncols != K and D->nrows != P->nrows.
 *
 * Aliasing (checked last; -1, "overlap" in gf2_last_error).  There is no in-place call: D may share no word with P.  The address
 * range of dist (P->nrows ints) may meet neither P's address range nor D's, and no table (2^r words) may meet D's range or dist's. */
#ifndef M4RI_HIP_COVER_H
#define M4RI_HIP_COVER_H
#include "m4ri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GF2_COVER_MAX_N = 32, GF2_COVER_MAX_R = 12, GF2_COVER_MAX_CODES = 16, GF2_COVER_MAX_SEGS = 256,
       GF2_COVER_MAX_LEADERS = 16384 /* sum of 2^r over the codes that have a table */ };
typedef struct { int n, k; uint32_t h[GF2_COVER_MAX_R]; } gf2_cover_code;   /* 56 bytes, host */
enum { GF2_COVER_IDENTITY, GF2_COVER_DROP, GF2_COVER_REPETITION, GF2_COVER_HAMMING, GF2_COVER_GOLAY23 };

/* host, no device: *code = the named code (see above); -1 for an unknown kind or a param outside its range */
int gf2_cover_code_named(int kind, int param, gf2_cover_code *code);

/* host, no device: leaders[0 .. 2^r) = the coset leaders of *code, *radius (may be NULL) their largest weight */
int gf2_cover_leaders(gf2_cover_code const *code, uint32_t *leaders, int *radius);

/* The reduction (see above).  codes, seg_code: HOST.  leaders: HOST array of ncodes DEVICE pointers.  dist: DEVICE int32[P->nrows]
 * or NULL. */
int gf2_cover_reduce_dev(gf2_dmat *D, gf2_dmat const *P, int c0, gf2_cover_code const *codes, int ncodes,
                         const unsigned char *seg_code, int nseg, const uint32_t *const *leaders, int *dist, void *stream);

/* without a device: returns the kernel variant (0: every lane reads the words of its row from global memory, 1: the window words of a
 * workgroup's rows are first copied into LDS), -1 for a bad argument (the rules of gf2_cover_reduce_dev on codes, seg_code and the
 * window's length); out[0] = threads per workgroup, out[1] = LDS bytes (at most 160 KiB), out[2] = rows per workgroup and pass,
 * out[3] = lanes per row of the copy, out[4] = K, out[5] = the window's bits, out[6] = table words, out[7] = workgroups.  out may be
 * NULL. */
int gf2_cover_plan(int nrows, int p_ncols, gf2_cover_code const *codes, int ncodes, const unsigned char *seg_code, int nseg,
                   long long out[8]);

#ifdef __cplusplus
}
#endif
#endif
