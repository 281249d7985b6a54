// attn_varlen.hip — ragged-batch (varlen) attention over the paged KV caches (lc_attn_varlen_paged_f16 / _kv8): ONE call for a
// continuous-batching step — a few prompts or prefill chunks of different lengths next to many sequences that decode one token — instead of a
// call per group of equal Nq or one call left-padded to the longest.
//   - Q and O are token-major [T, H, D]: the tokens of the step packed one sequence behind the other, sequence b owning rows
//     q0 = clamp(cu_q[b], 0, T) ... q0 + Nq_b - 1 with Nq_b = clamp(cu_q[b + 1] - q0, 0, min(max_nq, T - q0)).  cu_q (device int32[B + 1]) is
//     read by the kernel only, like kv_len: a captured graph replays with the offsets of its time.  The clamps are the memory-safety contract:
//     no value in cu_q makes a kernel read or write outside the T rows
//   - the grid is FlashAttention's varlen grid: B x Hkv x RB x S workgroups with RB = ceil(G max_nq / 64) from the HOST's bound max_nq; a
//     workgroup whose row block starts at or past R_b = G Nq_b returns before it touches LDS or a barrier
//   - everything else is the shared body (attn_decode_body.inc, VARLEN = true, LOCAL = true): inside a (sequence, K / V head) the rows keep the
//     head-major order r = g Nq_b + i, so row blocks, L_blk, tile_lo, the range partition and the bits are the chunk / local kernels'; only the
//     address of a row differs.  window = 0, sinks = nullptr is the widest window and no sink
//   - S > 1: the partials are indexed by the global row (total_rows = T H), and attn_varlen_combine_kernel<D> merges them for the tokens from
//     cu_q[0] to cu_q[B] - 1 only: the rows in front of the first sequence and behind the last are not written, with S = 1 and with S > 1 alike
// RB = 1: attn_varlen_paged_kernel<D, RT> / attn_varlen_paged_kv8_kernel<D, RT>; RB > 1: attn_varlen_chunk_paged_kernel<D> / _kv8_kernel<D>.
// There is no contiguous-cache form: a ragged batch only exists on a paged cache.
#pragma once
#include "attn_decode.hip"

namespace lc {

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv, int Nq,
                                                                int Ncap, int causal, int S, float sl2, long total_rows, int num_pages, int lps,
                                                                int max_pages, int window, const float* __restrict__ sinks,
                                                                const int* __restrict__ cu_q, int T_rows) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
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
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                      const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                      const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                      float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                      int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                      int num_pages, int lps, int max_pages, int window,
                                                                      const float* __restrict__ sinks, const int* __restrict__ cu_q, int T_rows) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
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
__global__ __launch_bounds__(256) void attn_varlen_paged_kv8_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                    const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                    const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                    float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                    int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                    int num_pages, int lps, int max_pages, int window,
                                                                    const float* __restrict__ sinks, const int* __restrict__ cu_q, int T_rows) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
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
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kv8_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                          const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                          const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                          const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                          float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                          int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                          int num_pages, int lps, int max_pages, int window,
                                                                          const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                          int T_rows) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
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

// attn_decode_combine_kernel<D> for a ragged call: the same merge of the S partials, in the same order (same bits), for the rows of the tokens
// clamp(cu_q[0], 0, T) ... clamp(cu_q[B], 0, T) - 1 — the range kernels wrote no partial for a token outside them, and its O row is nobody's.
// (A row between those bounds that no sequence owns — a cu_q that is not monotone, a sequence longer than max_nq — merges whatever the workspace
// holds into its own O row: garbage in, garbage out, in bounds.)
template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                  half_t* __restrict__ O, const int* __restrict__ cu_q, int B, int T_rows, int H,
                                                                  int S) {
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
  half4_t y = {(half_t)(acc[0] * inv), (half_t)(acc[1] * inv), (half_t)(acc[2] * inv), (half_t)(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * D + d) = y;
}

}  // namespace lc
