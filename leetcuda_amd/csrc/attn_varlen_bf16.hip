// attn_varlen_bf16.hip — the ragged-batch kernels of attn_varlen.hip for bfloat16 Q, O and 16-bit pools (lc_attn_varlen_paged_bf16 / _kv8_bf16;
// DESIGN.md §4.3m).  The shared body with BF16 = true, which changes four places and nothing else:
//   - Sᵀ = K Qᵀ and Oᵀ += Vᵀ Pᵀ run on v_mfma_f32_16x16x32_bf16 (mfma16_16<true>); the fragments travel as raw 16-bit lanes, so loads, the LDS
//     images and the transposed reads are the fp16 kernels'
//   - P is rounded to bf16 (RNE, v_cvt_pk_bf16_f32); l keeps summing the unrounded fp32 p
//   - O is rounded once, fp32 -> bf16 RNE, in the S = 1 store and in attn_varlen_combine_bf16_kernel
//   - an fp8 cache: e4m3 -> bf16 in registers (kv8_bf16x8, exact); the pools are the bytes the fp16 kernels read and the scales stay in fp32
// The mask, the ranges, the page and cu_q clamps, the sinks and (m, l) are the body's: fp32, untouched.  The pointers are half_t*: 16-bit lanes
// that only the MFMA and the two conversions interpret.
#pragma once
#include "attn_varlen.hip"

namespace lc {

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_bf16_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                     const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                     const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                     float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                     int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                     int num_pages, int lps, int max_pages, int window,
                                                                     const float* __restrict__ sinks, const int* __restrict__ cu_q, int T_rows) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_bf16_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                           const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                           const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                           float* __restrict__ part_o, float* __restrict__ part_lse, int H,
                                                                           int Hkv, int Nq, int Ncap, int causal, int S, float sl2,
                                                                           long total_rows, int num_pages, int lps, int max_pages, int window,
                                                                           const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                           int T_rows) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_kv8_bf16_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                         const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                         const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                         const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                         float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                         int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                         int num_pages, int lps, int max_pages, int window,
                                                                         const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                         int T_rows) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  // (the body takes the pools as byte bases only: page_base)
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kv8_bf16_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                               const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                               const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                               const float* __restrict__ k_scale,
                                                                               const float* __restrict__ v_scale, float* __restrict__ part_o,
                                                                               float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap,
                                                                               int causal, int S, float sl2, long total_rows, int num_pages,
                                                                               int lps, int max_pages, int window, const float* __restrict__ sinks,
                                                                               const int* __restrict__ cu_q, int T_rows) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

// attn_varlen_combine_kernel<D> with a bf16 O: the same merge of the S fp32 partials in the same order for the same rows, and ONE rounding
// fp32 -> bf16 (RNE) at the store.  A kernel of its own, statement for statement the fp16 one: that kernel keeps its source and its code
template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_bf16_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                       half_t* __restrict__ O, const int* __restrict__ cu_q, int B, int T_rows,
                                                                       int H, int S) {
  constexpr int TPR = D / 4;   // threads per row
  const long row = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  const int d = (threadIdx.x % TPR) * 4;
  const int beg = cu_q[0], end = cu_q[B];
  const long total_rows = (long)T_rows * H;
  if (row < (long)(beg < 0 ? 0 : (beg > T_rows ? T_rows : beg)) * H) return;
  if (row >= (long)(end < 0 ? 0 : (end > T_rows ? T_rows : end)) * H) return;
  float mx = DEC_NEG_INF;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, part_lse[(long)s * total_rows + row]);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  float ws = 0.f;
  if (mx != DEC_NEG_INF) {
    for (int s = 0; s < S; ++s) {
      const float wgt = __builtin_amdgcn_exp2f(part_lse[(long)s * total_rows + row] - mx);
      if (wgt > 0.f) {
        acc += *reinterpret_cast<const f32x4_t*>(part_o + ((long)s * total_rows + row) * D + d) * wgt;
        ws += wgt;
      }
    }
  }
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  half4_t y = {cvt16<true>(acc[0] * inv), cvt16<true>(acc[1] * inv), cvt16<true>(acc[2] * inv), cvt16<true>(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * D + d) = y;
}

}  // namespace lc
