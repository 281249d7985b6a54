// mla_index_topk.hip — the slot selection of the lightning indexer (lc_mla_index_topk): for every query token t the pool
// slots of the min(n_t, topk) largest of its n_t visible index logits, in ASCENDING key position, the rest of the row -1.  n_t comes from cu_q /
// kv_len / the causal flag exactly as in mla_index_logits.hip, never from the logits.  The order is the IEEE totalOrder of the fp32 bit
// patterns (-0 < +0, a NaN sorts by sign and payload), lower position first among equal patterns: the output is a pure function of the input.
//
//   - one workgroup of 1024 threads (16 wave64) per row; the owner of the row is found by all threads over cu_q (the largest b that owns it)
//   - n_t <= topk: no selection, positions 0 .. n_t - 1 are translated and written
//   - else a RADIX SELECT on the order-preserving key (sign set: all bits flipped, else the sign bit set) in THREE passes of 11, 11 and 10
//     bits, the most significant first: a 2048-bin LDS histogram (LDS atomics) of the digit over the columns that match the prefix found so
//     far, then a scan of the bins from the top finds the digit where the count of larger keys crosses `need`.  After the last pass the
//     prefix is the threshold pattern thr and `need` the number of columns EQUAL to thr that are still wanted.  32-bit counters
//   - then ONE ordered compaction pass in chunks of 4096 columns (a wave 256 consecutive ones, four coalesced 4-byte loads a lane): keep
//     key > thr, or key == thr among the first `need` equals of the row.  Per wave eight ballots and popcounts give every kept column its
//     rank inside the wave; the waves' (greater, equal) counts of a chunk go through LDS (two alternating sets: one barrier a chunk) and the
//     totals are carried from chunk to chunk in registers.  Position of a kept column: greater before it + min(equal before it, need)
//   - the row is read four times, from L2 after the first; only columns j < n_t are ever read
//   - translation: clamp(block_table[b, j / page_size], 0, num_pages - 1) page_size + j % page_size, the clamp of the logits kernel
#pragma once
#include "lc_common.h"

namespace lc {

constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int TOPK_BINS = 2048;             // 11-bit digits
constexpr int TOPK_CHUNK = 4 * TOPK_THREADS;

LC_DEVINL unsigned topk_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }

// exclusive prefix sum of v over the 1024 threads in thread order; wtot: 16 LDS words (free again when the call returns)
LC_DEVINL unsigned topk_block_scan(unsigned v, unsigned* wtot, int lane, int w) {
  unsigned incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wtot[w] = incl;
  __syncthreads();
  unsigned base = 0;
  for (int i = 0; i < w; ++i) base += wtot[i];
  __syncthreads();
  return base + incl - v;
}

__global__ __launch_bounds__(TOPK_THREADS) void mla_index_topk_kernel(const float* __restrict__ logits, int* __restrict__ slots,
                                                                      const int* __restrict__ cu_q, const int* __restrict__ block_table,
                                                                      const int* __restrict__ kv_len, int B, int T, int max_nq,
                                                                      int num_pages, int lps, int max_pages, long ld, int topk, int causal) {
  __shared__ unsigned hist[TOPK_BINS];
  __shared__ unsigned wtot[TOPK_WAVES];
  __shared__ unsigned wcnt[2][TOPK_WAVES][2];   // [set][wave]{greater, equal} of a compaction chunk
  __shared__ int owner;
  __shared__ unsigned found[2];                 // {digit, need} of a pass
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int t = blockIdx.x;
  int* __restrict__ out = slots + (long)t * topk;   // (T topk <= 2^31 - 1)

  // ---- the row's sequence: the largest b with q0_b <= t < q0_b + Nq_b (clamps of the attention entries); -1: nobody's
  if (tid == 0) owner = -1;
  for (int i = tid; i < TOPK_BINS; i += TOPK_THREADS) hist[i] = 0;
  __syncthreads();
  for (int b = tid; b < B; b += TOPK_THREADS) {
    const int c0 = cu_q[b], c1 = cu_q[b + 1];
    const int q0 = c0 < 0 ? 0 : (c0 > T ? T : c0);
    const int cap = max_nq < T - q0 ? max_nq : T - q0;
    const int Nqb = c1 <= q0 ? 0 : (c1 - q0 > cap ? cap : c1 - q0);
    if (t >= q0 && t < q0 + Nqb) atomicMax(&owner, b);
  }
  __syncthreads();
  const int b = owner;   // (uniform)
  int n = 0;
  if (b >= 0) {
    const int c0 = cu_q[b], c1 = cu_q[b + 1];
    const int q0 = c0 < 0 ? 0 : (c0 > T ? T : c0);
    const int cap = max_nq < T - q0 ? max_nq : T - q0;
    const int Nqb = c1 <= q0 ? 0 : (c1 - q0 > cap ? cap : c1 - q0);
    const int Ncap = max_pages << lps;
    int Lb = kv_len[b];
    Lb = Lb < 0 ? 0 : (Lb > Ncap ? Ncap : Lb);
    const int v = causal ? Lb - Nqb + (t - q0) + 1 : Lb;
    n = v < 0 ? 0 : (v > Lb ? Lb : v);
  }
  const int pmask = (1 << lps) - 1;
  auto slot_of = [&](int j) {   // (j < n <= L_b: a table position below ceil(L_b / page_size))
    int id = block_table[(long)b * max_pages + (j >> lps)];
    id = id < 0 ? 0 : (id < num_pages ? id : num_pages - 1);
    return (id << lps) + (j & pmask);
  };
  const int total = n < topk ? n : topk;
  for (int i = total + tid; i < topk; i += TOPK_THREADS) out[i] = -1;
  if (n <= topk) {
    for (int j = tid; j < n; j += TOPK_THREADS) out[j] = slot_of(j);
    return;
  }
  const unsigned* __restrict__ row = reinterpret_cast<const unsigned*>(logits + (long)t * ld);

  // ---- radix select: after pass p the top bits of thr are known, `need` columns are still wanted among the keys that match them
  unsigned thr = 0, known = 0, need = (unsigned)topk;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const int shift = p == 0 ? 21 : (p == 1 ? 10 : 0);
    const unsigned dmask = p == 2 ? 0x3ffu : 0x7ffu;
    for (int j0 = 0; j0 < n; j0 += TOPK_CHUNK) {
      unsigned key[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + e * TOPK_THREADS + tid;
        key[e] = topk_key(row[j < n ? j : n - 1]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j0 + e * TOPK_THREADS + tid < n && (key[e] & known) == thr) atomicAdd(&hist[(key[e] >> shift) & dmask], 1u);
    }
    __syncthreads();
    // thread i owns the digits 2047 - 2 i and 2046 - 2 i: an exclusive scan in thread order counts the keys with a larger digit
    const unsigned hi = hist[TOPK_BINS - 1 - 2 * tid], lo = hist[TOPK_BINS - 2 - 2 * tid];
    const unsigned above = topk_block_scan(hi + lo, wtot, lane, w);   // (its barriers: every thread has read its bins)
    hist[TOPK_BINS - 1 - 2 * tid] = 0;
    hist[TOPK_BINS - 2 - 2 * tid] = 0;
    if (above < need && need <= above + hi) {
      found[0] = TOPK_BINS - 1 - 2 * tid;
      found[1] = need - above;
    } else if (above + hi < need && need <= above + hi + lo) {
      found[0] = TOPK_BINS - 2 - 2 * tid;
      found[1] = need - above - hi;
    }
    __syncthreads();
    thr |= found[0] << shift;
    known |= dmask << shift;
    need = found[1];
    __syncthreads();   // (found is rewritten by the next pass)
  }

  // ---- ordered compaction: wave w of a chunk owns columns j0 + 256 w + 64 e + lane, e = 0 .. 3
  const unsigned long below = (1ul << lane) - 1;
  unsigned gt_carry = 0, eq_carry = 0;
  int set = 0;
  for (int j0 = 0; j0 < n; j0 += TOPK_CHUNK, set ^= 1) {
    unsigned key[4];
    const int jw = j0 + 256 * w + lane;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = jw + 64 * e;
      key[e] = topk_key(row[j < n ? j : n - 1]);
    }
    unsigned gt_before[4], eq_before[4], gt_w = 0, eq_w = 0;
    bool is_gt[4], is_eq[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = jw + 64 * e < n;
      is_gt[e] = in && key[e] > thr;
      is_eq[e] = in && key[e] == thr;
      const unsigned long bg = __builtin_amdgcn_ballot_w64(is_gt[e]), be = __builtin_amdgcn_ballot_w64(is_eq[e]);
      gt_before[e] = gt_w + (unsigned)__builtin_popcountl(bg & below);
      eq_before[e] = eq_w + (unsigned)__builtin_popcountl(be & below);
      gt_w += (unsigned)__builtin_popcountl(bg);
      eq_w += (unsigned)__builtin_popcountl(be);
    }
    if (lane == 0) {
      wcnt[set][w][0] = gt_w;
      wcnt[set][w][1] = eq_w;
    }
    __syncthreads();   // (the other set is written next: one barrier a chunk)
    unsigned gt_base = gt_carry, eq_base = eq_carry;
    for (int i = 0; i < TOPK_WAVES; ++i) {
      const unsigned g = wcnt[set][i][0], q = wcnt[set][i][1];
      if (i < w) {
        gt_base += g;
        eq_base += q;
      }
      gt_carry += g;
      eq_carry += q;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned eqr = eq_base + eq_before[e];   // how many equals of the row stand in front of this column
      if (is_gt[e] || (is_eq[e] && eqr < need)) out[gt_base + gt_before[e] + (eqr < need ? eqr : need)] = slot_of(jw + 64 * e);
    }
  }
}

}  // namespace lc
