// attn_merge.hip — merge two attention results over DISJOINT key sets into the result over their union (lc_attn_merge_states_f16 / _bf16;
// DESIGN.md §4.3n): what joins the prefix level and the suffix level of a shared-prefix (cascade) step, two KV shards, or a windowed and a
// global pass.  A state is (O [T,H,D] 16-bit, lse float[T H]): the normalised output of a row and the natural log of its softmax denominator,
// as the lc_attn_varlen_paged_lse_* entries write them.  Per row, in fp32:
//   m = max(la, lb);  wa = exp(la - m), wb = exp(lb - m)
//   O = (wa Oa + wb Ob) / (wa + wb), rounded ONCE to the 16-bit type (RNE);  lse = m + log(wa + wb)
//   la = lb = -inf (neither side met a key): O = 0, lse = -inf
// One side -inf: its weight is exp(-inf) = 0 and the other's is exp(0) = 1, the sum is 1 and log 1 = 0 — the other state passes through bit for
// bit, O and lse (a weight of exactly 0 drops its O without reading a number into it: a row that met no key may hold anything).
// Layout: a lane owns 16 bytes (8 elements) of a row, the D / 8 lanes of a row sit in ONE wave, 256 / (D / 8) rows per workgroup.
// Aliasing: Oout may be Oa or Ob and lse_out may be lse_a or lse_b (no pointer here is __restrict__).  A lane reads and writes its own 16 bytes
// of O only; every lane of a row reads the row's two lse values BEFORE the row's one lse store — the loads are the first statements of the row,
// the store is the last, and the lanes of a row execute both in lockstep in one wave: no lane can read what the store wrote.
// cu_q (optional): with cu_q != nullptr only the rows of tokens clamp(cu_q[0], 0, T) ... clamp(cu_q[B], 0, T) - 1 are touched — the rows the
// ragged calls own — so that a captured step whose T is a bound keeps the rows behind its last token.
#pragma once
#include "attn_decode.hip"

namespace lc {

// one raw 16-bit lane -> fp32 (exact): fp16, or bfloat16 by a shift
template <bool BF16>
LC_DEVINL float cvt32(half_t x) {
  if constexpr (BF16)
    return __builtin_bit_cast(float, (uint32_t)__builtin_bit_cast(uint16_t, x) << 16);
  else
    return (float)x;
}

template <int D, bool BF16>
LC_DEVINL void merge_states_row(const half_t* Oa, const float* lse_a, const half_t* Ob, const float* lse_b, half_t* Oout, float* lse_out,
                                const int* cu_q, int B, int T_rows, int H) {
  constexpr int LPR = D / 8;   // lanes per row
  const long row = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const int d = (threadIdx.x % LPR) * 8;
  long lo = 0, hi = (long)T_rows * H;
  if (cu_q) {
    const int beg = cu_q[0], end = cu_q[B];
    lo = (long)(beg < 0 ? 0 : (beg > T_rows ? T_rows : beg)) * H;
    hi = (long)(end < 0 ? 0 : (end > T_rows ? T_rows : end)) * H;
  }
  if (row < lo || row >= hi) return;
  const float la = lse_a[row], lb = lse_b[row];   // (both read by every lane of the row, in front of the row's lse store below)
  const half8_t xa = *reinterpret_cast<const half8_t*>(Oa + row * D + d);
  const half8_t xb = *reinterpret_cast<const half8_t*>(Ob + row * D + d);
  const float m = fmaxf(la, lb);
  const float mu = (m == DEC_NEG_INF) ? 0.f : m;   // neither side met a key: both weights are exp(-inf) = 0
  const float wa = __builtin_amdgcn_exp2f((la - mu) * 1.4426950408889634f);
  const float wb = __builtin_amdgcn_exp2f((lb - mu) * 1.4426950408889634f);
  const float ws = wa + wb;
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  half8_t y;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = cvt32<BF16>(xa[e]), b = cvt32<BF16>(xb[e]);
    // (a weight of 0 leaves the other side's value, weight 1 and sum 1, untouched: x 1, / 1)
    const float x = wb == 0.f ? (wa == 0.f ? 0.f : a) : (wa == 0.f ? b : (wa * a + wb * b) * inv);
    y[e] = cvt16<BF16>(x);
  }
  *reinterpret_cast<half8_t*>(Oout + row * D + d) = y;
  if (d == 0) lse_out[row] = ws > 0.f ? m + log2f(ws) * 0.6931471805599453f : DEC_NEG_INF;
}

template <int D>
__global__ __launch_bounds__(256) void attn_merge_states_kernel(const half_t* Oa, const float* lse_a, const half_t* Ob, const float* lse_b,
                                                                half_t* Oout, float* lse_out, const int* cu_q, int B, int T_rows, int H) {
  merge_states_row<D, false>(Oa, lse_a, Ob, lse_b, Oout, lse_out, cu_q, B, T_rows, H);
}

template <int D>
__global__ __launch_bounds__(256) void attn_merge_states_bf16_kernel(const half_t* Oa, const float* lse_a, const half_t* Ob, const float* lse_b,
                                                                     half_t* Oout, float* lse_out, const int* cu_q, int B, int T_rows,
                                                                     int H) {
  merge_states_row<D, true>(Oa, lse_a, Ob, lse_b, Oout, lse_out, cu_q, B, T_rows, H);
}

}  // namespace lc
