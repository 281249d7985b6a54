// attn_chunk.hip — chunked-prefill attention over the KV caches (lc_attn_chunk_f16 / _paged_f16 / _paged_kv8): the decode calls
// of §4.3e / f / g with the bound R = G x Nq <= 64 removed.  A wave cannot hold more than four row tiles of 16 (the register file: <128,4> is at
// 417 .. 423 VGPR + AGPR), so the way past 64 rows is more workgroups, not more rows per workgroup:
//   - RB = ceil(R / 64) row blocks per (batch, K / V head); the 1-D grid is B x Hkv x RB x S, index ((b Hkv + kvh) RB + rb) S + s — the blocks
//     and ranges of one (b, kvh) are adjacent: they re-read the same K / V run, which should meet in L2
//   - block rb owns rows 64 rb ... min(R, 64 rb + 64) - 1 of the contiguous [R, D] matrix of its (b, kvh) (row r = g Nq + i, as in decode); rows
//     >= R load row R - 1 and store nothing; a block may straddle a head boundary (Nq % 64 != 0): the mask takes i = r % Nq from the GLOBAL row
//   - causal: a block walks only the tiles some row of it can see.  L_blk = clamp(L_b - Nq + i_max + 1, 0, L_b), i_max = the block's last token
//     (Nq - 1 where the block straddles); tiles, range partition, the source clamp and "a step past the end" follow L_blk, the mask follows L_b.
//     A block of an aligned call (Nq % 64 == 0) is thereby the decode call on its 64 query rows with kv_len = L_blk, bit for bit
// Everything inside a block is the decode body (attn_decode_body.inc, CHUNK = true, RT = 4): clamped sources, scalar table reads with prefetch,
// the select-on-index mask, the fp8 conversion in registers, the fp32 partials of split-KV (merged by attn_decode_combine_kernel<D>).
// Each block streams its visible K / V again: the call serves what attn_fwd_w4u_causal_kernel cannot (Nq != Nk, paged and fp8 caches), not its rate.
#pragma once
#include "attn_decode.hip"

namespace lc {

template <int D>
__global__ __launch_bounds__(256) void attn_chunk_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
                                                         half_t* __restrict__ O, const int* __restrict__ kv_len, float* __restrict__ part_o,
                                                         float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap, int causal, int S,
                                                         float sl2, long total_rows) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = false;
  const DecodeLocal lc{};
  constexpr bool PAGED = false;
  const DecodePaging pg{};
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
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
__global__ __launch_bounds__(256) void attn_chunk_paged_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                               const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                               const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                               float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv, int Nq,
                                                               int Ncap, int causal, int S, float sl2, long total_rows, int num_pages, int lps,
                                                               int max_pages) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = false;
  const DecodeLocal lc{};
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
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
__global__ __launch_bounds__(256) void attn_chunk_paged_kv8_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                   const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                   const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                   const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                   float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                   int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                   int num_pages, int lps, int max_pages) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = false;
  const DecodeLocal lc{};
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
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

}  // namespace lc
