// rope_append_varlen_bf16.hip — rope_append_varlen.hip for bfloat16 sources, Qout and 16-bit pools (lc_rope_append_varlen_bf16 / _kv8_bf16;
// DESIGN.md §4.3m).  The body is rope_append_varlen_body itself — the lane map, the binary search of cu_q, the clamps and the drop rules — with
// BF16 = true, which puts rope_rotate8_bf16 (rope_append_paged.hip) and kv8_quantize8_bf16 (kv_append_paged.hip) in place of the fp16 functions:
//   - a bf16 element IS the upper half of its fp32 value: the decode is a shift, exact, denormals included
//   - the arithmetic is rope_fma, the fp16 kernels' one rounded product and one fma in fp32, then ONE rounding to bf16 (RNE, v_cvt_pk_bf16_f32;
//     bf16 denormals are fp32 denormals and are kept).  Elements at or behind rot_dim, and all of V, are copied bit for bit
//   - fp8 pools: code = e4m3fn_rne(clamp(fp32(x) / s, -448, 448)) with the true division, taken of the rotated row ROUNDED TO bf16 first, so
//     that the pool equals what a bf16 pool quantised afterwards would hold.  A NaN is found on the bf16 bits ((h & 0x7fff) > 0x7f80) and on the
//     quotient; its code gets 0x7F or-ed in.  +-inf gives +-448
// The fp16 flavours (rope_rotate8, kv8_quot2, kv8_quantize8) stay what they are; the bf16 ones are defined next to them.
#pragma once
#include "rope_append_varlen.hip"

namespace lc {

// grid and arguments: rope_append_varlen_kernel's; every 16-bit element is a bf16
template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_varlen_bf16_kernel(const half_t* Q, const half_t* __restrict__ Knew,
                                                                      const half_t* __restrict__ Vnew, half_t* Qout, half_t* __restrict__ Kpool,
                                                                      half_t* __restrict__ Vpool, const float* __restrict__ cos_sin,
                                                                      const int* __restrict__ cu_q, const int* __restrict__ block_table,
                                                                      const int* __restrict__ kv_len, int B, int H, int Hkv, int T, int max_nq,
                                                                      int num_pages, int lps, int max_pages, int nblk, int rot_dim, int max_pos,
                                                                      long long q_row_stride, long long kv_row_stride) {
  rope_append_varlen_body<D, INTERLEAVED, false, true>(Q, Knew, Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr, B,
                                                       H, Hkv, T, max_nq, num_pages, lps, max_pages, nblk, rot_dim, max_pos, q_row_stride,
                                                       kv_row_stride);
}

template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_varlen_kv8_bf16_kernel(const half_t* Q, const half_t* __restrict__ Knew,
                                                                          const half_t* __restrict__ Vnew, half_t* Qout,
                                                                          uint8_t* __restrict__ Kpool8, uint8_t* __restrict__ Vpool8,
                                                                          const float* __restrict__ cos_sin, const int* __restrict__ cu_q,
                                                                          const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                                          const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                          int B, int H, int Hkv, int T, int max_nq, int num_pages, int lps,
                                                                          int max_pages, int nblk, int rot_dim, int max_pos,
                                                                          long long q_row_stride, long long kv_row_stride) {
  rope_append_varlen_body<D, INTERLEAVED, true, true>(Q, Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale,
                                                      B, H, Hkv, T, max_nq, num_pages, lps, max_pages, nblk, rot_dim, max_pos, q_row_stride,
                                                      kv_row_stride);
}

}  // namespace lc
