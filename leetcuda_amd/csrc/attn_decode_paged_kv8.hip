// attn_decode_paged_kv8.hip — decode attention over a paged KV cache kept in fp8 (lc_attn_decode_paged_kv8):
// attn_decode_paged_kernel<D, RT> (attn_decode_paged.hip) with the cache element an OCP e4m3fn byte and one fp32 scale per K / V head,
//   O = softmax(Q (k_scale[g] K8)ᵀ / sqrt(D)) (v_scale[g] V8).
// The call is bound by reading K and V once, so the lever is the size of what is read: half the bytes, the same arithmetic.
//   - Kpool8 / Vpool8 are [num_pages, Hkv, page_size, D] bytes; page, table, clamps and the SGPR page base + 32-bit VGPR offset are §4.3f's
//   - K: a lane's D / 4 contiguous elements are D / 4 bytes (two dwordx4 at D = 128, one at D = 64); bytes 8 s ... 8 s + 7 become the half8 A
//     operand of k-step s right in front of its MFMA (kv8_half8: one v_cvt_scalef32_pk_f16_fp8 per two elements, scale 1.0, exact)
//   - V: a 16-byte chunk is 16 elements of one key row, a 64-lane chunk group 8 (D = 128) or 16 (D = 64) key rows — inside one 16-key block, so
//     the page stays wave-uniform; the chunk is converted when it is written to the per-wave LDS image, as the two adjacent fp16 chunks of its
//     row under the image's swizzle.  The image, its transposed reads and the P V phase are the fp16 kernels'
//   - scales, fp32 only: k_scale[g] is multiplied once into the score scale, v_scale[g] into the 1 / l that normalises O (fp16 output and fp32
//     partial alike); both are read through a uniform address.  Only the kernel reads them: a captured graph may be replayed after they changed
//   - a byte of a position >= L_b is never read (source rows are clamped to L_b - 1), so NaN codes (0x7f, 0xff) in the tail do not matter
// With power-of-two scales every step is the fp16 kernel's on the dequantised pool, bit for bit: the converted K / V are that pool's values
// divided by the scale, which the fp32 accumulations carry exactly, and the scale comes back in one fp32 multiplication that commutes with
// the rounding.  Partition, mask, softmax, merge and epilogues are the shared body (attn_decode_body.inc, KV8 = true).
#pragma once
#include "attn_decode.hip"

namespace lc {

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_decode_paged_kv8_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                    const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                    const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                    float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                    int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                    int num_pages, int lps, int max_pages) {
  constexpr bool CHUNK = false;
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
