// rope_append_varlen_pos.hip — rope_append_varlen.hip / rope_append_varlen_bf16.hip with the rotary position of every token stated by the caller
// (lc_rope_append_varlen_pos_f16 / _kv8 / _bf16 / _kv8_bf16).  The nodes of a draft tree sit in neighbouring cache slots, but a
// node's rotary position is prefix length + depth: siblings share one.  The body is rope_append_varlen_body itself with POS = true, which
// changes ONE thing: the cos_sin row of token t is clamp(pos_ids[t], 0, max_pos - 1) in place of clamp(p, 0, max_pos - 1).  The cache slot
// p = L_b - Nq_b + i, the p < 0 rule, dropped tokens, quantisation, strides and in-place Q are the twin's; pos_ids[t] = p for every token gives
// the twin's bytes.  pos_ids (device int32[T]) is read only for a token that a sequence owns.
#pragma once
#include "rope_append_varlen_bf16.hip"

namespace lc {

// grid and arguments: rope_append_varlen_kernel's, with pos_ids behind them
template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_varlen_pos_kernel(const half_t* Q, const half_t* __restrict__ Knew,
                                                                     const half_t* __restrict__ Vnew, half_t* Qout, half_t* __restrict__ Kpool,
                                                                     half_t* __restrict__ Vpool, const float* __restrict__ cos_sin,
                                                                     const int* __restrict__ cu_q, const int* __restrict__ block_table,
                                                                     const int* __restrict__ kv_len, int B, int H, int Hkv, int T, int max_nq,
                                                                     int num_pages, int lps, int max_pages, int nblk, int rot_dim, int max_pos,
                                                                     long long q_row_stride, long long kv_row_stride,
                                                                     const int* __restrict__ pos_ids) {
  rope_append_varlen_body<D, INTERLEAVED, false, false, true>(Q, Knew, Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr,
                                                              B, H, Hkv, T, max_nq, num_pages, lps, max_pages, nblk, rot_dim, max_pos, q_row_stride,
                                                              kv_row_stride, pos_ids);
}

template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_varlen_pos_kv8_kernel(const half_t* Q, const half_t* __restrict__ Knew,
                                                                         const half_t* __restrict__ Vnew, half_t* Qout,
                                                                         uint8_t* __restrict__ Kpool8, uint8_t* __restrict__ Vpool8,
                                                                         const float* __restrict__ cos_sin, const int* __restrict__ cu_q,
                                                                         const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                                         const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                         int B, int H, int Hkv, int T, int max_nq, int num_pages, int lps,
                                                                         int max_pages, int nblk, int rot_dim, int max_pos, long long q_row_stride,
                                                                         long long kv_row_stride, const int* __restrict__ pos_ids) {
  rope_append_varlen_body<D, INTERLEAVED, true, false, true>(Q, Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale,
                                                             B, H, Hkv, T, max_nq, num_pages, lps, max_pages, nblk, rot_dim, max_pos, q_row_stride,
                                                             kv_row_stride, pos_ids);
}

// ... every 16-bit element a bf16
template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_varlen_pos_bf16_kernel(const half_t* Q, const half_t* __restrict__ Knew,
                                                                          const half_t* __restrict__ Vnew, half_t* Qout,
                                                                          half_t* __restrict__ Kpool, half_t* __restrict__ Vpool,
                                                                          const float* __restrict__ cos_sin, const int* __restrict__ cu_q,
                                                                          const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                                          int B, int H, int Hkv, int T, int max_nq, int num_pages, int lps,
                                                                          int max_pages, int nblk, int rot_dim, int max_pos, long long q_row_stride,
                                                                          long long kv_row_stride, const int* __restrict__ pos_ids) {
  rope_append_varlen_body<D, INTERLEAVED, false, true, true>(Q, Knew, Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr,
                                                             B, H, Hkv, T, max_nq, num_pages, lps, max_pages, nblk, rot_dim, max_pos, q_row_stride,
                                                             kv_row_stride, pos_ids);
}

template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_varlen_pos_kv8_bf16_kernel(const half_t* Q, const half_t* __restrict__ Knew,
                                                                              const half_t* __restrict__ Vnew, half_t* Qout,
                                                                              uint8_t* __restrict__ Kpool8, uint8_t* __restrict__ Vpool8,
                                                                              const float* __restrict__ cos_sin, const int* __restrict__ cu_q,
                                                                              const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                                              const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                              int B, int H, int Hkv, int T, int max_nq, int num_pages, int lps,
                                                                              int max_pages, int nblk, int rot_dim, int max_pos,
                                                                              long long q_row_stride, long long kv_row_stride,
                                                                              const int* __restrict__ pos_ids) {
  rope_append_varlen_body<D, INTERLEAVED, true, true, true>(Q, Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale,
                                                            B, H, Hkv, T, max_nq, num_pages, lps, max_pages, nblk, rot_dim, max_pos, q_row_stride,
                                                            kv_row_stride, pos_ids);
}

}  // namespace lc
