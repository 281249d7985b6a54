// attn_decode.hip — decode attention over a KV cache (lc_attn_decode_f16): Nq new query tokens per sequence, G = H / Hkv
// query heads per K / V head, R = G x Nq <= 64 query rows per (batch, K / V head) against L_b = kv_len[b] cached keys.
//
// The problem is bound by reading K and V ONCE from HBM, so nothing here is shared between waves and nothing is read twice:
//   - one workgroup (4 wave64) per (batch, K / V head, KV range s of S); the range partition is computed IN THE KERNEL from L_b
//     (T_b = ceil(L_b / 64) tiles, range s = tiles [s T_b / S, (s + 1) T_b / S)): the host never sees kv_len, a range may be empty
//   - wave w owns the 64-key tiles t0 + w, t0 + w + 4, ... of the range and keeps its own online softmax (running max, sum, fp32 O); there is
//     no workgroup barrier inside the key loop, and ONE merge of the four (m, l, O) through LDS behind it
//   - K goes straight from global memory into MFMA-operand registers: Sᵀ = K Qᵀ on v_mfma_f32_16x16x32_f16 with the K rows as the A operand;
//     lane (key = lane & 15, h = lane >> 4) reads the D / 4 CONTIGUOUS halves d = h D / 4 ... of its key row (64 bytes at D = 128) and k-step s
//     takes elements 8 s ... 8 s + 7 of them — Q is read from its LDS image under the same permutation of d, so the sum is over every d once
//   - Sᵀ leaves each lane with ONE query row (lane & 15) and 16 keys of the tile: P in fp16 is, register for register, the B operand of
//     Oᵀ = Vᵀ Pᵀ (no shuffle); the A operand Vᵀ comes from a per-wave row-major LDS image of the V tile through ds_read_b64_tr_b16.  The next
//     tile's K and V loads are issued (into registers) behind the current tile's softmax, and V is copied to the image at the end of the
//     iteration: the loads of a whole tile (32 KiB at D = 128) are in flight per wave while it computes
//   - masking is a SELECT on the key index before the row maximum (a score may be NaN); K / V source rows are clamped to <= L_b - 1 and never
//     zero-filled, so a masked P = 0 never meets a NaN of the cache tail and every address stays inside [0, Ncap) (the rule of §4.2c)
//   - rows R ... 16 RT - 1 of the padded row tiles load Q row R - 1 and store nothing
//   - S == 1: the workgroup normalises and writes fp16 O.  S > 1: it writes the NORMALISED fp32 partial O and the row's log-sum-exp in the
//     log2 domain (-inf: the range held no visible key) to the workspace; attn_decode_combine_kernel<D> merges the S partials (weight 0 for
//     an empty range, O = 0 when every range is empty)
// Reproducibility: the bits of one (batch, K / V head) depend on its Q, K, V, L_b, Nq, the causal flag and S only.
// The body is shared with the paged-cache kernel (attn_decode_paged.hip), which replaces the address of a key row and nothing else,
// and with the fp8-cache kernel (attn_decode_paged_kv8.hip, §4.3g), which loads bytes and converts them in registers.
#pragma once
#include <type_traits>

#include "lc_common.h"

namespace lc {

constexpr int DEC_KVB = 64;      // keys per tile
constexpr int DEC_WAVES = 4;
constexpr float DEC_NEG_INF = -__builtin_inff();

// byte offset of 16-byte chunk `ch` of key row `row` in the per-wave V image (rows of D halves, chunks XOR-swizzled by the row so that the
// four rows of a transposed 4 x 16 block read fall on different banks)
template <int D>
LC_DEVINL int dec_v_off(int row, int ch) {
  if constexpr (D == 128) return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  else return 128 * row + 16 * (ch ^ (((row & 3) << 1) | ((row >> 2) & 1)));
}

template <int D, int RT>
struct DecodeLds {
  static constexpr int kQStride = D * 2 + 16;                  // bytes per Q row: 16 bytes of padding spread the 16 rows of a fragment read over the banks
  static constexpr int kQBytes = 16 * RT * kQStride;
  static constexpr int kVBytes = DEC_KVB * D * 2;              // one wave's V image (a step of 64 keys; the merge slots need it whole)
  static constexpr int kOBytes = RT * (D / 16) * 4 * 64 * 4;   // one wave's O accumulators (merge)
  static constexpr int kMlOff = kQBytes;                       // m[4][16 RT], l[4][16 RT]
  static constexpr int kMlBytes = 2 * DEC_WAVES * 16 * RT * 4;
  static constexpr int kVOff = kMlOff + kMlBytes;
  static constexpr int kTotal = kVOff + DEC_WAVES * kVBytes;   // (the merge re-uses the V images: two slots of kOBytes <= 4 kVBytes)
  static_assert(2 * kOBytes <= DEC_WAVES * kVBytes, "merge slots must fit the V images");
};

// Where a logical key row lives.  Contiguous cache: K / V are [B,Hkv,Ncap,D] and every field here is unused.  Paged cache (attn_decode_paged.hip;
// DESIGN.md §4.3f): K / V are pools [num_pages,Hkv,page_size,D], logical keys p page_size ... of batch entry b sit in pool page table[b][p].
struct DecodePaging {
  const int* table;   // device int32[B, max_pages]
  int num_pages, lps, max_pages;   // lps = log2(page_size), page_size >= 16
};

// An fp8 cache (attn_decode_paged_kv8.hip): K / V pool elements are OCP e4m3fn bytes, the value of element x of K / V head g is
// k_scale[g] x (v_scale[g] x).  The fp16 kernels leave every field unused.
struct DecodeKv8 {
  const float *k_scale, *v_scale;   // device float[Hkv] or nullptr (= 1.0)
};

// A sliding window and attention sinks (attn_local.hip).  Every other kernel leaves both fields unused.
struct DecodeLocal {
  int window;           // W > 0: a row whose last visible key is p sees keys p - W + 1 .. p; 0: no lower edge
  const float* sinks;   // device float[H], one logit per query head in natural units (not scaled by 1 / sqrt(D)), or nullptr
};

// A ragged batch (attn_varlen.hip): Q and O are token-major [T, H, D] and cu_q holds the row offsets of the sequences.  Every
// other kernel leaves both fields unused.
struct DecodeVarlen {
  const int* cu_q;   // device int32[B + 1]; read by the kernel only, every value clamped into [0, T]
  int T;             // rows of Q and O
};

// The row's log-sum-exp next to O (attn_varlen.hip).  Every other kernel leaves the field unused.
struct DecodeLse {
  float* lse;   // device float[rows of O]: ln(sum over the row's visible keys of exp(score), the sink included); -inf: no key, no sink
};

// A look-back visibility mask per query token (attn_varlen.hip).  Every other kernel leaves the field unused.
struct DecodeTree {
  const uint64_t* mask;   // device uint64[T]: bit d of word t lets token t, at cache slot p, see key p - d (d < 64); keys 64 or more slots back are not governed
};

// eight e4m3 bytes (a: bytes 0 .. 3, b: bytes 4 .. 7, memory order) as eight fp16 values, element i = byte i: one v_cvt_scalef32_pk_f16_fp8 per two
// elements, scale 1.0 — every e4m3 value is an fp16 value (the smallest, 2^-9, a normal one), so the conversion is exact; 0x7f / 0xff give NaN
LC_DEVINL u32x4_t kv8_half8(uint32_t a, uint32_t b) {
  return u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(a, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(a, 1.0f, true)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(b, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(b, 1.0f, true))};
}

// ... and as eight bf16 values (v_cvt_scalef32_pk_bf16_fp8, scale 1.0): exact as well — an e4m3 value has 4 significand bits and an exponent
// far inside bf16's range
LC_DEVINL u32x4_t kv8_bf16x8(uint32_t a, uint32_t b) {
  return u32x4_t{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false)),
                 __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true))};
}
// The element flavour of the shared body (attn_decode_body.inc, `BF16`): the e4m3 -> 16-bit conversion and the 16 x 16 x 32 MFMA on raw
// 16-bit fragments, on the model of lc_common.h's mfma32_16 / cvt16.  BF16 = false: kv8_half8 and mfma16 themselves.
template <bool BF16>
LC_DEVINL u32x4_t kv8_16x8(uint32_t a, uint32_t b) {
  if constexpr (BF16) return kv8_bf16x8(a, b);
  else return kv8_half8(a, b);
}
template <bool BF16>
LC_DEVINL f32x4_t mfma16_16(half8_t a, half8_t b, f32x4_t c) {
  if constexpr (BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else
    return mfma16(a, b, c);
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
                                                          half_t* __restrict__ O, const int* __restrict__ kv_len, float* __restrict__ part_o,
                                                          float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap, int causal, int S,
                                                          float sl2, long total_rows) {
  constexpr bool CHUNK = false;
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

// O[row] = sum_s w_s part_o[s][row] / sum_s w_s with w_s = exp2(lse_s - max lse): weight 0 for a range without a visible key (lse = -inf),
// O = 0 when no range has one.  One thread per (row, four d).
template <int D>
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                  half_t* __restrict__ O, long total_rows, int S) {
  constexpr int TPR = D / 4;   // threads per row
  const long row = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  const int d = (threadIdx.x % TPR) * 4;
  if (row >= total_rows) return;
  float mx = DEC_NEG_INF;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, part_lse[(long)s * total_rows + row]);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  float ws = 0.f;
  if (mx != DEC_NEG_INF) {
    for (int s = 0; s < S; ++s) {
      const float wgt = __builtin_amdgcn_exp2f(part_lse[(long)s * total_rows + row] - mx);
      if (wgt > 0.f) {   // (an empty range's partial is 0, but it is never read: weight 0 is not a multiplication)
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
