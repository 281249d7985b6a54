// attn_varlen_tree.hip — the ragged-batch kernels of attn_varlen_lse.hip with a look-back visibility mask per query token
// (lc_attn_varlen_paged_tree_f16 / _tree_kv8 / _tree_bf16 / _tree_kv8_bf16): the verification step of tree-structured
// speculative decoding, where the new tokens of a sequence are the nodes of a draft tree laid out in neighbouring cache slots and a node must
// see the prefix and its own ancestors, never its siblings.
// The shared body with LSE = true and TREE = true.  tree_mask is a device uint64[T], one word per token row of Q.  Token i of sequence b sits at
// slot p = L_b - Nq_b + i; key j is visible iff the twin's rule holds (j <= p, and j > p - W under a window) AND, for d = p - j in [0, 64), bit d
// of the token's word is set.  Bit 0 is the token's own key; keys 64 or more slots back are not governed.
//   - a word of all ones IS the twin: the same select, the same bits in O and lse — a decoding or prefilling sequence rides in the same batch
//   - a row whose word hides every key is a row without a visible key: O = 0 and lse = -inf, or the sink alone
//   - the mask only removes keys: the tiles a workgroup walks, the KV ranges, the page ids and the clamps are the twin's, and so is the plan
//   - a step whose every key lies 64 or more slots below the workgroup's lowest row slot takes the twin's select (a wave-uniform branch): a long
//     cache pays for the bit test in its last tiles only
// Each kernel takes its LSE twin's arguments with `tree_mask` behind `lse`.  S > 1 is merged by attn_varlen_combine_lse_kernel<D> / _lse_bf16_kernel<D>.
#pragma once
#include "attn_varlen_lse.hip"

namespace lc {

// (the argument lists of the LSE twins, fp16 / bf16 pools and fp8 pools)
#define LC_TREE_ARGS16                                                                                                                         \
  const half_t *__restrict__ Q, const half_t *__restrict__ Kpool, const half_t *__restrict__ Vpool, half_t *__restrict__ O,                    \
      const int *__restrict__ kv_len, const int *__restrict__ block_table, float *__restrict__ part_o, float *__restrict__ part_lse, int H,    \
      int Hkv, int Nq, int Ncap, int causal, int S, float sl2, long total_rows, int num_pages, int lps, int max_pages, int window,             \
      const float *__restrict__ sinks, const int *__restrict__ cu_q, int T_rows, float *__restrict__ lse, const uint64_t *__restrict__ tree_mask
#define LC_TREE_ARGS8                                                                                                                          \
  const half_t *__restrict__ Q, const uint8_t *__restrict__ Kpool8, const uint8_t *__restrict__ Vpool8, half_t *__restrict__ O,                \
      const int *__restrict__ kv_len, const int *__restrict__ block_table, const float *__restrict__ k_scale,                                  \
      const float *__restrict__ v_scale, float *__restrict__ part_o, float *__restrict__ part_lse, int H, int Hkv, int Nq, int Ncap,           \
      int causal, int S, float sl2, long total_rows, int num_pages, int lps, int max_pages, int window, const float *__restrict__ sinks,       \
      const int *__restrict__ cu_q, int T_rows, float *__restrict__ lse, const uint64_t *__restrict__ tree_mask
// (what every tree kernel states in front of the body, behind CHUNK, KV8 and BF16)
#define LC_TREE_COMMON                                           \
  constexpr bool LOCAL = true;                                   \
  constexpr bool PAGED = true;                                   \
  constexpr bool VARLEN = true;                                  \
  constexpr bool LSE = true;                                     \
  constexpr bool TREE = true;                                    \
  const DecodePaging pg{block_table, num_pages, lps, max_pages}; \
  const DecodeLocal lc{window, sinks};                           \
  const DecodeVarlen vl{cu_q, T_rows};                           \
  const DecodeLse ls{lse};                                       \
  const DecodeTree tr{tree_mask};
#define LC_TREE_POOL16                   \
  const DecodeKv8 kv8{};                 \
  const half_t* __restrict__ K = Kpool;  \
  const half_t* __restrict__ V = Vpool;
// (the body takes the pools as byte bases only: page_base)
#define LC_TREE_POOL8                                                        \
  const DecodeKv8 kv8{k_scale, v_scale};                                     \
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);   \
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_tree_kernel(LC_TREE_ARGS16) {
  constexpr bool CHUNK = false;
  constexpr bool KV8 = false;
  constexpr bool BF16 = false;
  LC_TREE_COMMON
  LC_TREE_POOL16
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_tree_kernel(LC_TREE_ARGS16) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool KV8 = false;
  constexpr bool BF16 = false;
  LC_TREE_COMMON
  LC_TREE_POOL16
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_kv8_tree_kernel(LC_TREE_ARGS8) {
  constexpr bool CHUNK = false;
  constexpr bool KV8 = true;
  constexpr bool BF16 = false;
  LC_TREE_COMMON
  LC_TREE_POOL8
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kv8_tree_kernel(LC_TREE_ARGS8) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool KV8 = true;
  constexpr bool BF16 = false;
  LC_TREE_COMMON
  LC_TREE_POOL8
#include "attn_decode_body.inc"
}

// ---- the bfloat16 forms (BF16 = true: attn_varlen_bf16.hip's four places, and the same mask)

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_tree_bf16_kernel(LC_TREE_ARGS16) {
  constexpr bool CHUNK = false;
  constexpr bool KV8 = false;
  constexpr bool BF16 = true;
  LC_TREE_COMMON
  LC_TREE_POOL16
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_tree_bf16_kernel(LC_TREE_ARGS16) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool KV8 = false;
  constexpr bool BF16 = true;
  LC_TREE_COMMON
  LC_TREE_POOL16
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_kv8_tree_bf16_kernel(LC_TREE_ARGS8) {
  constexpr bool CHUNK = false;
  constexpr bool KV8 = true;
  constexpr bool BF16 = true;
  LC_TREE_COMMON
  LC_TREE_POOL8
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kv8_tree_bf16_kernel(LC_TREE_ARGS8) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool KV8 = true;
  constexpr bool BF16 = true;
  LC_TREE_COMMON
  LC_TREE_POOL8
#include "attn_decode_body.inc"
}

#undef LC_TREE_ARGS16
#undef LC_TREE_ARGS8
#undef LC_TREE_COMMON
#undef LC_TREE_POOL16
#undef LC_TREE_POOL8

}  // namespace lc
