// attn_local.hip — sliding-window and attention-sink attention over the three KV caches (lc_attn_local_f16 / _paged_f16 / _paged_kv8; DESIGN.md
// §4.3k): the decode and chunk kernels of §4.3e / f / g / i with two more arguments, for the models whose layers attend to the last W keys only
// (Mistral-class, Gemma 2 / 3, gpt-oss) and whose heads carry a learned sink logit (gpt-oss).
//   - window = W > 0 (causal calls only): the query at position p = L_b - Nq + i sees keys p - W < j <= p, W keys with its own, clipped at key 0.
//     A workgroup starts at the tile of the lowest key any of its rows sees, tile_lo = max(0, L_b - Nq + i_min + 1 - W) / 64, and it is the
//     tiles [tile_lo, T) that are cut into the S ranges: what is streamed is the window, not the cache.  Tiles below tile_lo are never loaded
//     and no block-table entry below them is read.  The mask stays a select on the key index: one unsigned compare of j - lim + W against W
//   - sinks = device float[H] or nullptr: sinks[h] is one more logit of every row of query head h — in natural units, NOT multiplied by
//     1 / sqrt(D) — that takes part in the softmax denominator and contributes no value.  It is where the running (m, l) of range 0, wave 0 start
//     (m = sink log2 e, l = 1, O = 0); the wave merge, the fp32 partial with its log-sum-exp and attn_decode_combine_kernel<D> need no change.
//     -inf is no sink; a row with a sink and no visible key is O = 0
// Everything else is the shared body (attn_decode_body.inc, LOCAL = true).  A call with a window whose low edge falls on a tile seam is, bit
// for bit, the decode call on the cache rows [L_b - W, L_b) with kv_len = W: same tiles per wave, same range partition.
// R <= 64: attn_local_*_kernel<D, RT>, the decode kernels' grid; R > 64: attn_local_chunk_*_kernel<D>, the chunk kernels' grid of row blocks.
#pragma once
#include "attn_decode.hip"

namespace lc {

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_local_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
                                                         half_t* __restrict__ O, const int* __restrict__ kv_len, float* __restrict__ part_o,
                                                         float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap, int causal, int S,
                                                         float sl2, long total_rows, int window, const float* __restrict__ sinks) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = false;
  const DecodePaging pg{};
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
  const DecodeLocal lc{window, sinks};
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_local_chunk_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K,
                                                               const half_t* __restrict__ V, half_t* __restrict__ O,
                                                               const int* __restrict__ kv_len, float* __restrict__ part_o,
                                                               float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap, int causal, int S,
                                                               float sl2, long total_rows, int window, const float* __restrict__ sinks) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = false;
  const DecodePaging pg{};
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
  const DecodeLocal lc{window, sinks};
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_local_paged_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                               const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                               const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                               float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv, int Nq,
                                                               int Ncap, int causal, int S, float sl2, long total_rows, int num_pages, int lps,
                                                               int max_pages, int window, const float* __restrict__ sinks) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_local_chunk_paged_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                     const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                     const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                     float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                     int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                     int num_pages, int lps, int max_pages, int window,
                                                                     const float* __restrict__ sinks) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_local_paged_kv8_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                   const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                   const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                   const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                   float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                   int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                   int num_pages, int lps, int max_pages, int window,
                                                                   const float* __restrict__ sinks) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  // (the body takes the pools as byte bases only: page_base)
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_local_chunk_paged_kv8_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                         const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                         const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                         const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                         float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                         int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                         int num_pages, int lps, int max_pages, int window,
                                                                         const float* __restrict__ sinks) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

}  // namespace lc
