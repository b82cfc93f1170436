// gf2_join_select.inc -- the weight-filtered join (include/m4ri_hip_join_select.h; host side: join_host.cpp; plan: join_plan.h;
// DESIGN.md section 7.15.1).  Included by gf2_join.hip inside its anonymous namespace, behind the join's own kernels, whose helpers it
// uses: the pairs and their order are those of gf2_join_scatter_kernel, but only the HITS -- the pairs whose XOR has between wlo and whi
// ones in the columns [wc0, wc1) -- leave the kernel.  Two passes over the pairs, and no scratch that grows with their number:
//
//     the hits of every run of A, one long long per run (twice: the scan below overwrites one)   gf2_join_weigh_kernel<1 | 2 | 8 | 64 lanes per pair>
//     hit sums -> hit offsets, *hits                                                             gf2_join_scan_kernel (gf2_join.hip)
//     D[hit offset + rank] = A[..] ^ B[..], ia, ib, wt for the hits alone                        gf2_join_select_scatter_kernel<1 | 2 | 8 | 64 lanes per row>
//
// The weigh pass forms only the words of A ^ B that hold a column of the range, so its lanes per pair follow the words of the range; the
// scatter weighs every output again with the lanes of the row store, ranks the hits of a round in output order (a ballot inside the
// wave, the waves' sums through LDS, a running total) and XORs whole rows for the hits only.
//
// Integer arithmetic, one writer per output word, nothing that depends on the order in which waves arrive: two runs give the same bits.

// ---- word-level helpers: plain values and pointers, no thread index (tests/test_join_select_helpers_cpu.py runs their text on the CPU)

// the first word of a row that holds a column of [wc0, wc1), and one past the last; an empty range holds no word: both are 0
__device__ __forceinline__ long long join_select_first_word(int wc0, int wc1) { return wc0 < wc1 ? (long long)(wc0 >> 6) : 0; }
__device__ __forceinline__ long long join_select_end_word(int wc0, int wc1) { return wc0 < wc1 ? (long long)((wc1 - 1) >> 6) + 1 : 0; }

// is a pair of weight w a hit of the window [wlo, whi]?
__device__ __forceinline__ int join_select_is_hit(int w, int wlo, int whi) { return w >= wlo && w <= whi; }

// the ones of a ^ p in the columns [wc0, wc1) that lane `sub` of `lanes` counts: the range's words go in pairs (words 2u and 2u + 1, one
// 16-byte access where the operand allows it: gf2_load2), pair sub, sub + lanes, ... of the pairs that meet the range.  nw: the words of
// a row; no word from nw on is read, and a word of the row outside the range counts nothing
__device__ __forceinline__ int join_select_pair_weight(const u64 *a, const u64 *p, long long nw, int vec_a, int vec_b, int sub, int lanes, int wc0,
                                                       int wc1) {
  const long long u1 = (join_select_end_word(wc0, wc1) + 1) >> 1;
  int w = 0;
  for (long long u = (join_select_first_word(wc0, wc1) >> 1) + sub; u < u1; u += lanes) {
    const long long k = 2 * u;
    if (k + 1 < nw) {
      u64 x0, x1, y0, y1;
      gf2_load2(a, k, vec_a, x0, x1);
      gf2_load2(p, k, vec_b, y0, y1);
      w += gf2_word_weight(x0 ^ y0, k, wc0, wc1) + gf2_word_weight(x1 ^ y1, k + 1, wc0, wc1);
    } else {
      w += gf2_word_weight(a[k] ^ p[k], k, wc0, wc1);
    }
  }
  return w;
}

// ---- the kernels

// what a run knows of its outputs, in LDS: the sums of the partner counts before every position and the first partner of every position
// (the prologue of gf2_join_scatter_kernel).  -> the run's outputs.  Every lane calls it; barriers lie inside, the last one at its end
__device__ __forceinline__ long long join_select_run_outputs(const int *ska, long long na, const int *skb, long long nb, long long s0, int *stage,
                                                             int *span, long long *wave_sum, long long *pre, int *lpos) {
  int l[kJoinRunItems], c[kJoinRunItems];
  join_run_partners(ska, na, skb, nb, s0, stage, span, l, c);
  long long mine = 0, total;
#pragma unroll
  for (int i = 0; i < kJoinRunItems; ++i) mine += c[i];
  long long before = gf2_block_scan<long long, kJoinWaves>(mine, wave_sum, &total);
#pragma unroll
  for (int i = 0; i < kJoinRunItems; ++i) {
    const int q = kJoinRunItems * threadIdx.x + i;
    pre[q] = before;
    lpos[q] = l[i];
    before += c[i];
  }
  __syncthreads();
  return total;
}

// hsums[run] = hown[run] = the hits of the run.  The outputs are dealt to groups of LANES lanes as the scatter deals them
template <int LANES>
__global__ void __launch_bounds__(kJoinThreads) gf2_join_weigh_kernel(const u64 *A, long long lda, const u64 *B, long long ldb, int ncols,
                                                                      const int *order_a, const int *ska, long long na, const int *order_b,
                                                                      const int *skb, long long nb, long long *hsums, long long *hown, int wc0,
                                                                      int wc1, int wlo, int whi, int vec_a, int vec_b) {
  __shared__ long long pre[kJoinRunRows];
  __shared__ int lpos[kJoinRunRows];
  __shared__ int stage[kJoinSpanKeys];
  __shared__ int span[2];
  __shared__ long long wave_sum[kJoinWaves];
  const long long s0 = (long long)blockIdx.x * kJoinRunRows;
  const long long total = join_select_run_outputs(ska, na, skb, nb, s0, stage, span, wave_sum, pre, lpos);
  const long long nw = ((long long)ncols + 63) >> 6;
  const int sub = threadIdx.x % LANES;
  long long mine = 0;
  for (long long j = threadIdx.x / LANES; j < total; j += kJoinThreads / LANES) {  // the lanes of a group share j: they leave together
    const int q = gf2_find_position(pre, kJoinRunRows, j);
    const long long p = lpos[q] + (j - pre[q]);
    const int a = order_a[s0 + q], r = order_b[p];
    int w = join_select_pair_weight(A + (long long)a * lda, B + (long long)r * ldb, nw, vec_a, vec_b, sub, LANES, wc0, wc1);
#pragma unroll
    for (int d = LANES >> 1; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);  // over the lane group
    if (sub == 0 && join_select_is_hit(w, wlo, whi)) ++mine;
  }
  long long hits;
  gf2_block_scan<long long, kJoinWaves>(mine, wave_sum, &hits);  // wave_sum is free: the scan of the outputs read it before the last barrier of the prologue
  if (threadIdx.x == 0) {
    hsums[blockIdx.x] = hits;
    hown[blockIdx.x] = hits;
  }
}

// A run with hits below the capacity walks its outputs in rounds of kJoinThreads / LANES, one output per lane group, and weighs each one
// again.  The hits of a round are ranked in output order: the lanes of a wave hold consecutive outputs, so a hit's rank inside its wave
// is the number of hits in the lanes before its group (a ballot), and the waves' numbers of hits go through LDS -- two rows, used in
// turn, so that one barrier per round is enough: a wave writes row k & 1 for round k + 2 only behind the barrier of round k + 1, which
// every wave reaches only after it has read row k & 1 for round k.  Every lane holds the same running total `done`, so every lane
// leaves the loop in the same round: when the run's own hits, or those that the capacity has room for, are written.
template <int LANES>
__global__ void __launch_bounds__(kJoinThreads) gf2_join_select_scatter_kernel(
    const u64 *A, long long lda, const u64 *B, long long ldb, int ncols, const int *order_a, const int *ska, long long na, const int *order_b,
    const int *skb, long long nb, const long long *hoffs, const long long *hown, u64 *D, long long ldd, long long cap, int *ia, int *ib, int *wt,
    int wc0, int wc1, int wlo, int whi, int vec_a, int vec_b, int vec_d) {
  __shared__ long long pre[kJoinRunRows];
  __shared__ int lpos[kJoinRunRows];
  __shared__ int stage[kJoinSpanKeys];
  __shared__ int span[2];
  __shared__ long long wave_sum[kJoinWaves];
  __shared__ int wave_hits[2][kJoinWaves];
  const long long own = hown[blockIdx.x], hoff = hoffs[blockIdx.x];
  if (own == 0 || hoff >= cap) return;  // no hit, or every hit behind the capacity: not a key of the run is read
  const long long s0 = (long long)blockIdx.x * kJoinRunRows;
  const long long total = join_select_run_outputs(ska, na, skb, nb, s0, stage, span, wave_sum, pre, lpos);
  const long long limit = own < cap - hoff ? own : cap - hoff;  // the hits of this run that are written
  const long long nw = ((long long)ncols + 63) >> 6;
  const u64 mlast = ~0ull >> (63 - (int)(((long long)ncols - 1) & 63));
  const int sub = threadIdx.x % LANES, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long long done = 0;  // the hits of the rounds before this one: the same in every lane
  int round = 0;
  for (long long j0 = 0; j0 < total && done < limit; j0 += kJoinThreads / LANES, round ^= 1) {
    const long long j = j0 + threadIdx.x / LANES;
    int a = 0, r = 0, w = 0;
    if (j < total) {
      const int q = gf2_find_position(pre, kJoinRunRows, j);
      const long long p = lpos[q] + (j - pre[q]);
      a = order_a[s0 + q];
      r = order_b[p];
      w = join_select_pair_weight(A + (long long)a * lda, B + (long long)r * ldb, nw, vec_a, vec_b, sub, LANES, wc0, wc1);
    }
#pragma unroll
    for (int d = LANES >> 1; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);  // over the lane group; every lane of the wave is here
    const bool hit = j < total && join_select_is_hit(w, wlo, whi);
    const unsigned long long firsts = __ballot(hit && sub == 0);  // one bit per hit of this wave, at the first lane of its group
    if (lane == 0) wave_hits[round][wave] = __popcll(firsts);
    __syncthreads();
    long long rank = done + __popcll(firsts & ((1ull << (lane - sub)) - 1ull));
    int all = 0;
#pragma unroll
    for (int wv = 0; wv < kJoinWaves; ++wv) {
      const int n = wave_hits[round][wv];
      if (wv < wave) rank += n;
      all += n;
    }
    done += all;
    if (hit && rank < limit) {
      const long long at = hoff + rank;
      if (D) join_xor_row<LANES>(D + at * ldd, A + (long long)a * lda, B + (long long)r * ldb, nw, mlast, vec_a, vec_b, vec_d, sub, 0, 0);
      if (sub == 0) {
        if (ia) ia[at] = a;
        if (ib) ib[at] = r;
        if (wt) wt[at] = w;
      }
    }
  }
}

}  // namespace: the launchers below are extern "C" and must not lie inside it (gf2_join.hip's closing brace ends the one reopened below)

#define JOIN_WEIGH(LANES)                                                                                                               \
  hipLaunchKernelGGL((gf2_join_weigh_kernel<LANES>), grid, block, 0, stream, A, lda, B, ldb, ncols, order_a, skeys_a, (long long)nrows_a, \
                     order_b, skeys_b, (long long)nrows_b, hsums, hown, wc0, wc1, wlo, whi, vec_a, vec_b)

extern "C" hipError_t gf2k_join_weigh(const u64 *A, long long lda, int nrows_a, const u64 *B, long long ldb, int nrows_b, int ncols,
                                      const int *order_a, const int *skeys_a, const int *order_b, const int *skeys_b, long long *hsums,
                                      long long *hown, long long *hits, int wc0, int wc1, int wlo, int whi, int lanes, hipStream_t stream) {
  const JoinSelectPlan plan = join_select_plan(nrows_a, nrows_b, ncols, 0, wc0, wc1);
  if (plan.join.passes < 0 || nrows_a <= 0 || nrows_b <= 0) return hipErrorInvalidValue;
  if (lanes < 0) lanes = plan.weigh_lanes;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_a = gf2_rows_aligned16(A, lda, nrows_a, nw), vec_b = gf2_rows_aligned16(B, ldb, nrows_b, nw);
  const dim3 grid((unsigned)plan.join.runs), block(kJoinThreads);
  if (lanes == 1)
    JOIN_WEIGH(1);
  else if (lanes == 2)
    JOIN_WEIGH(2);
  else if (lanes == 8)
    JOIN_WEIGH(8);
  else if (lanes == 64)
    JOIN_WEIGH(64);
  else
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf2_join_scan_kernel, dim3(1), dim3(kJoinThreads), 0, stream, hsums, plan.join.runs, hits);
  return hipGetLastError();
}

#define JOIN_SELECT_SCATTER(LANES)                                                                                                      \
  hipLaunchKernelGGL((gf2_join_select_scatter_kernel<LANES>), grid, block, 0, stream, A, lda, B, ldb, ncols, order_a, skeys_a,          \
                     (long long)nrows_a, order_b, skeys_b, (long long)nrows_b, hoffs, hown, D, ldd, (long long)cap, ia, ib, wt, wc0, wc1, wlo, \
                     whi, vec_a, vec_b, vec_d)

extern "C" hipError_t gf2k_join_select_scatter(const u64 *A, long long lda, int nrows_a, const u64 *B, long long ldb, int nrows_b, int ncols,
                                               const int *order_a, const int *skeys_a, const int *order_b, const int *skeys_b,
                                               const long long *hoffs, const long long *hown, u64 *D, long long ldd, int cap, int *ia, int *ib,
                                               int *wt, int wc0, int wc1, int wlo, int whi, int lanes, hipStream_t stream) {
  const JoinSelectPlan plan = join_select_plan(nrows_a, nrows_b, ncols, 0, wc0, wc1);
  if (plan.join.passes < 0 || nrows_a <= 0 || nrows_b <= 0 || cap <= 0) return hipErrorInvalidValue;
  if (lanes < 0) lanes = plan.join.lanes;
  const long long nw = ((long long)ncols + 63) >> 6;
  const int vec_a = gf2_rows_aligned16(A, lda, nrows_a, nw), vec_b = gf2_rows_aligned16(B, ldb, nrows_b, nw),
            vec_d = D ? gf2_rows_aligned16(D, ldd, cap, nw) : 0;
  const dim3 grid((unsigned)plan.join.runs), block(kJoinThreads);
  if (lanes == 1)
    JOIN_SELECT_SCATTER(1);
  else if (lanes == 2)
    JOIN_SELECT_SCATTER(2);
  else if (lanes == 8)
    JOIN_SELECT_SCATTER(8);
  else if (lanes == 64)
    JOIN_SELECT_SCATTER(64);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

namespace {
