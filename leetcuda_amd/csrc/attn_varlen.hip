// attn_varlen.hip — ragged-batch (varlen) attention over the paged KV caches (lc_attn_varlen_paged_*): ONE call for a
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
//   - S > 1: the partials are indexed by the global row (total_rows = T H), and a combine kernel merges them for the tokens from cu_q[0] to
//     cu_q[B] - 1 only: the rows in front of the first sequence and behind the last are not written, with S = 1 and with S > 1 alike
// There is no contiguous-cache form: a ragged batch only exists on a paged cache.
//
// The family is ONE body and four flags, and twelve of their sixteen values exist.  A kernel's name states them:
//   attn_varlen_ [chunk_] paged_ [kv8_] [lse_ | tree_] [bf16_] kernel          RB = 1: <D, RT>; chunk, RB > 1: <D> (RT = 4)
// KV8 (§4.3l): the pools are e4m3 bytes, and k_scale, v_scale (fp32 [Hkv] or nullptr = 1.0) follow block_table; an fp16 / bf16 pool kernel takes
//   neither.
// BF16 (lc_attn_varlen_paged_*bf16; §4.3m): Q, O and 16-bit pools are bfloat16, which changes four places and nothing else:
//   - Sᵀ = K Qᵀ and Oᵀ += Vᵀ Pᵀ run on v_mfma_f32_16x16x32_bf16 (mfma16_16<true>); the fragments travel as raw 16-bit lanes, so loads, the LDS
//     images and the transposed reads are the fp16 kernels'
//   - P is rounded to bf16 (RNE, v_cvt_pk_bf16_f32); l keeps summing the unrounded fp32 p
//   - O is rounded once, fp32 -> bf16 RNE, in the S = 1 store and in the bf16 combine kernels
//   - an fp8 cache: e4m3 -> bf16 in registers (kv8_bf16x8, exact); the pools are the bytes the fp16 kernels read and the scales stay in fp32
//   The mask, the ranges, the page and cu_q clamps, the sinks and (m, l) are the body's: fp32, untouched.  The pointers are half_t*: 16-bit lanes
//   that only the MFMA and the two conversions interpret.
// LSE (lc_attn_varlen_paged_lse_*; §4.3n): the kernel also hands back each row's log-sum-exp, the softmax state a caller needs to merge two
//   attention results over disjoint key sets — a shared prefix and the private suffixes (cascade attention), KV shards, a window and a global
//   pass.  It adds ONE store and nothing else: where wave 0 writes a row's O (S = 1), the h = 0 lanes write
//     lse[row] = l > 0 ? (m + log2 l) ln 2 : -inf        row = t H + head, the global row of O
//   the NATURAL log of the sum of exp(score) over the row's visible keys, the sink included; score = q.k / sqrt(D) (x k_scale: fp8 pools), v_scale
//   does not enter.  With S > 1 the range kernels write part_lse as they always did and the _lse combine kernels store lse next to O.  O is the
//   twin's, bit for bit.  The kernel takes its twin's arguments with `lse` (device float[T H]) behind them; a plain kernel takes no `lse`.  Rows
//   nobody owns are written in neither buffer.
// TREE (lc_attn_varlen_paged_tree_*; §4.3o; always with LSE): a look-back visibility mask per query token, for the verification step of
//   tree-structured speculative decoding, where the new tokens of a sequence are the nodes of a draft tree laid out in neighbouring cache slots and
//   a node must see the prefix and its own ancestors, never its siblings.  tree_mask is a device uint64[T], one word per token row of Q, behind
//   `lse`.  Token i of sequence b sits at slot p = L_b - Nq_b + i; key j is visible iff the twin's rule holds (j <= p, and j > p - W under a
//   window) AND, for d = p - j in [0, 64), bit d of the token's word is set.  Bit 0 is the token's own key; keys 64 or more slots back are not
//   governed.
//   - a word of all ones IS the twin: the same select, the same bits in O and lse — a decoding or prefilling sequence rides in the same batch
//   - a row whose word hides every key is a row without a visible key: O = 0 and lse = -inf, or the sink alone
//   - the mask only removes keys: the tiles a workgroup walks, the KV ranges, the page ids and the clamps are the twin's, and so is the plan
//   - a step whose every key lies 64 or more slots below the workgroup's lowest row slot takes the twin's select (a wave-uniform branch): a long
//     cache pays for the bit test in its last tiles only
//   S > 1 is merged by the _lse combine kernels.
#pragma once
#include "attn_decode.hip"

namespace lc {

// VarlenKernels<KV8, BF16, LSE, TREE>: the two range kernels of those flags — ranges<D, RT>() (RB = 1) and chunk<D>() (RB > 1) — for the launcher
// (tu_attn_varlen_impl.h).  attn_varlen_pair.inc specialises it next to each pair, so a launcher cannot name a kernel of other flags
template <bool KV8, bool BF16, bool LSE, bool TREE>
struct VarlenKernels;

// What the 24 kernels share, stated once as text (a macro cannot hold the #include of the body, and the body has to be included: §4.3d, §4.3m).
// The argument lists of a kernel over 16-bit pools (..._false) and over fp8 pools (..._true), the optional tails behind T_rows ...
#define LC_VARLEN_ARGS_false                                                                                                                   \
  const half_t *__restrict__ Q, const half_t *__restrict__ Kpool, const half_t *__restrict__ Vpool, half_t *__restrict__ O,                    \
      const int *__restrict__ kv_len, const int *__restrict__ block_table, float *__restrict__ part_o, float *__restrict__ part_lse, int H,    \
      int Hkv, int Nq, int Ncap, int causal, int S, float sl2, long total_rows, int num_pages, int lps, int max_pages, int window,             \
      const float *__restrict__ sinks, const int *__restrict__ cu_q, int T_rows
#define LC_VARLEN_ARGS_true                                                                                                                    \
  const half_t *__restrict__ Q, const uint8_t *__restrict__ Kpool8, const uint8_t *__restrict__ Vpool8, half_t *__restrict__ O,                \
      const int *__restrict__ kv_len, const int *__restrict__ block_table, const float *__restrict__ k_scale,                                  \
      const float *__restrict__ v_scale, float *__restrict__ part_o, float *__restrict__ part_lse, int H, int Hkv, int Nq, int Ncap,           \
      int causal, int S, float sl2, long total_rows, int num_pages, int lps, int max_pages, int window, const float *__restrict__ sinks,       \
      const int *__restrict__ cu_q, int T_rows
#define LC_VARLEN_LSE_ARG_false
#define LC_VARLEN_LSE_ARG_true , float *__restrict__ lse
#define LC_VARLEN_TREE_ARG_false
#define LC_VARLEN_TREE_ARG_true , const uint64_t *__restrict__ tree_mask
// ... and what stands in front of the body, behind RT and CHUNK: the flags and the Decode... structs of the arguments there are
#define LC_VARLEN_POOL_false             \
  const DecodeKv8 kv8{};                 \
  const half_t* __restrict__ K = Kpool;  \
  const half_t* __restrict__ V = Vpool;
// (the body takes the pools as byte bases only: page_base)
#define LC_VARLEN_POOL_true                                                  \
  const DecodeKv8 kv8{k_scale, v_scale};                                     \
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);   \
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
#define LC_VARLEN_LSE_false const DecodeLse ls{};
#define LC_VARLEN_LSE_true const DecodeLse ls{lse};
#define LC_VARLEN_TREE_false const DecodeTree tr{};
#define LC_VARLEN_TREE_true const DecodeTree tr{tree_mask};
#define LC_VARLEN_SIGNATURE_(RANGES_, CHUNK_, KV8_, BF16_, LSE_, TREE_) LC_VARLEN_ARGS_##KV8_ LC_VARLEN_LSE_ARG_##LSE_ LC_VARLEN_TREE_ARG_##TREE_
#define LC_VARLEN_COMMON_(RANGES_, CHUNK_, KV8_, BF16_, LSE_, TREE_) \
  constexpr bool LOCAL = true;                                     \
  constexpr bool PAGED = true;                                     \
  constexpr bool VARLEN = true;                                    \
  constexpr bool KV8 = KV8_;                                       \
  constexpr bool BF16 = BF16_;                                     \
  constexpr bool LSE = LSE_;                                       \
  constexpr bool TREE = TREE_;                                     \
  const DecodePaging pg{block_table, num_pages, lps, max_pages};   \
  const DecodeLocal lc{window, sinks};                             \
  const DecodeVarlen vl{cu_q, T_rows};                             \
  LC_VARLEN_POOL_##KV8_ LC_VARLEN_LSE_##LSE_ LC_VARLEN_TREE_##TREE_
#define LC_VARLEN_RANGES_(RANGES_, CHUNK_, KV8_, BF16_, LSE_, TREE_) RANGES_
#define LC_VARLEN_CHUNK_(RANGES_, CHUNK_, KV8_, BF16_, LSE_, TREE_) CHUNK_
#define LC_VARLEN_FLAGS_(RANGES_, CHUNK_, KV8_, BF16_, LSE_, TREE_) KV8_, BF16_, LSE_, TREE_
#define LC_VARLEN_APPLY(M, ...) M(__VA_ARGS__)

// The twelve variants.  Each states LC_VARLEN_PAIR — its <D, RT> kernel, its <D> chunk twin, KV8, BF16, LSE, TREE (the literals true / false) —
// and attn_varlen_pair.inc defines the two kernels from it.  A new flag is one more element here, in LC_VARLEN_COMMON_ and in the body
#define LC_VARLEN_PAIR attn_varlen_paged_kernel, attn_varlen_chunk_paged_kernel, false, false, false, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_kv8_kernel, attn_varlen_chunk_paged_kv8_kernel, true, false, false, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_bf16_kernel, attn_varlen_chunk_paged_bf16_kernel, false, true, false, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_kv8_bf16_kernel, attn_varlen_chunk_paged_kv8_bf16_kernel, true, true, false, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_lse_kernel, attn_varlen_chunk_paged_lse_kernel, false, false, true, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_kv8_lse_kernel, attn_varlen_chunk_paged_kv8_lse_kernel, true, false, true, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_lse_bf16_kernel, attn_varlen_chunk_paged_lse_bf16_kernel, false, true, true, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_kv8_lse_bf16_kernel, attn_varlen_chunk_paged_kv8_lse_bf16_kernel, true, true, true, false
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_tree_kernel, attn_varlen_chunk_paged_tree_kernel, false, false, true, true
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_kv8_tree_kernel, attn_varlen_chunk_paged_kv8_tree_kernel, true, false, true, true
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_tree_bf16_kernel, attn_varlen_chunk_paged_tree_bf16_kernel, false, true, true, true
#include "attn_varlen_pair.inc"
#define LC_VARLEN_PAIR attn_varlen_paged_kv8_tree_bf16_kernel, attn_varlen_chunk_paged_kv8_tree_bf16_kernel, true, true, true, true
#include "attn_varlen_pair.inc"

#undef LC_VARLEN_ARGS_false
#undef LC_VARLEN_ARGS_true
#undef LC_VARLEN_LSE_ARG_false
#undef LC_VARLEN_LSE_ARG_true
#undef LC_VARLEN_TREE_ARG_false
#undef LC_VARLEN_TREE_ARG_true
#undef LC_VARLEN_POOL_false
#undef LC_VARLEN_POOL_true
#undef LC_VARLEN_LSE_false
#undef LC_VARLEN_LSE_true
#undef LC_VARLEN_TREE_false
#undef LC_VARLEN_TREE_true
#undef LC_VARLEN_SIGNATURE_
#undef LC_VARLEN_COMMON_
#undef LC_VARLEN_RANGES_
#undef LC_VARLEN_CHUNK_
#undef LC_VARLEN_FLAGS_
#undef LC_VARLEN_APPLY

// The four combine kernels: attn_varlen_combine.inc merges the S partials of a ragged call, by BF16 (the rounding of O) and LSE (the row's
// log-sum-exp next to O; a tree plan's combine is the LSE plan's).  Four kernels on one included body: each keeps its own code (§4.3m)
template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                  half_t* __restrict__ O, const int* __restrict__ cu_q, int B, int T_rows, int H,
                                                                  int S) {
  constexpr bool BF16 = false;
  constexpr bool LSE = false;
  constexpr float* lse = nullptr;
#include "attn_varlen_combine.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_bf16_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                       half_t* __restrict__ O, const int* __restrict__ cu_q, int B, int T_rows,
                                                                       int H, int S) {
  constexpr bool BF16 = true;
  constexpr bool LSE = false;
  constexpr float* lse = nullptr;
#include "attn_varlen_combine.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_lse_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                      half_t* __restrict__ O, const int* __restrict__ cu_q, int B, int T_rows,
                                                                      int H, int S, float* __restrict__ lse) {
  constexpr bool BF16 = false;
  constexpr bool LSE = true;
#include "attn_varlen_combine.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_lse_bf16_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                           half_t* __restrict__ O, const int* __restrict__ cu_q, int B,
                                                                           int T_rows, int H, int S, float* __restrict__ lse) {
  constexpr bool BF16 = true;
  constexpr bool LSE = true;
#include "attn_varlen_combine.inc"
}

// VarlenCombine<BF16, LSE>::kernel<D>(): the combine kernel of those flags, for the launcher
template <bool BF16, bool LSE>
struct VarlenCombine {
  template <int D>
  static auto kernel() {
    if constexpr (LSE && BF16) return attn_varlen_combine_lse_bf16_kernel<D>;   // (if constexpr: a unit emits the one kernel it names)
    else if constexpr (LSE) return attn_varlen_combine_lse_kernel<D>;
    else if constexpr (BF16) return attn_varlen_combine_bf16_kernel<D>;
    else return attn_varlen_combine_kernel<D>;
  }
};

}  // namespace lc
