// mla_index_append_fp8.hip — the write side of the fp8 index-key pool (lc_mla_index_append_fp8_f16 / _bf16): the step's new
// index keys Kinew [T,128] (16-bit rows behind the caller's norm, RoPE and Hadamard, a row stride in elements) are quantised per row and
// scattered through the block table into k8 [num_pages, page_size, 128] (e4m3fn codes) and ks [num_pages, page_size] (fp32), what
// mla_index_logits_fp8.hip reads.  The token rule is mla_append_paged.hip's (mla_token_owner): owner by a binary search of cu_q, position
// p = L_b - Nq_b + i under its clamps; p < 0, a page id outside [0, num_pages) or a token nobody owns writes nothing.
// Quantisation of a row x, fp32 throughout:
//   amax = max(max_d |x_d|, 1e-4)            (a NaN element does not enter the maximum: it is taken on the bit patterns)
//   s    = amax / 448                        (the correctly rounded division); pow2: s = 2^ceil(log2 s), exact on the bits — V3.2's ue8m0
//   code = e4m3fn_rne(clamp(x_d / s, -448, 448)), kv_append_paged.hip's quotient, clamp and NaN rule (kv8_quot2 / kv8_quot2_bf16)
// A WAVE OWNS A ROW: a lane its two elements (one dword), the maximum six cross-lane steps on the non-negative patterns (integer order =
// fp32 order), one 2-byte store a lane (128 contiguous bytes a wave), lane 0 the scale.  The token is wave-uniform, so the search, the page id
// and the row base are scalar work.  Four rows a workgroup; no LDS, no barrier.  Plain HIP with builtins; every store is a vector store.
#pragma once
#include "mla_append_paged.hip"   // mla_token_owner (kv_append_paged.hip: kv8_quot2, kv8_quot2_bf16, the NaN tests)

namespace lc {

// grid: ceil(T / 4) workgroups of 256; lps = log2(page_size)
template <bool BF16>
__global__ __launch_bounds__(256) void mla_index_append_fp8_kernel(const half_t* __restrict__ Kinew, uint8_t* __restrict__ K8,
                                                                   float* __restrict__ Ks, const int* __restrict__ cu_q,
                                                                   const int* __restrict__ block_table, const int* __restrict__ kv_len, int B,
                                                                   int T, int max_nq, int num_pages, int lps, int max_pages, long long row_stride,
                                                                   int pow2) {
  const unsigned lane = threadIdx.x & 63u;
  const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (t >= T) return;
  int b, p;
  if (!mla_token_owner(cu_q, kv_len, B, T, max_nq, max_pages << lps, t, b, p)) return;
  if (p < 0) return;
  const int pid = block_table[(size_t)b * max_pages + (p >> lps)];   // p < L <= ncap: inside the table row
  if ((unsigned)pid >= (unsigned)num_pages) return;                  // a bad page id drops the row
  const size_t prow = ((size_t)pid << lps) + (unsigned)(p & ((1 << lps) - 1));

  const uint32_t raw = *reinterpret_cast<const uint32_t*>(Kinew + (size_t)t * (size_t)row_stride + lane * 2);
  // |x| of the two elements as fp32 patterns, a NaN as 0
  uint32_t a0, a1;
  if constexpr (BF16) {
    a0 = nan_bits_bf16(raw) ? 0u : (raw << 16) & 0x7fffffffu;
    a1 = nan_bits_bf16(raw >> 16) ? 0u : raw & 0x7fff0000u;
  } else {
    const half2_t x = __builtin_bit_cast(half2_t, raw);
    a0 = nan_bits16(raw) ? 0u : __builtin_bit_cast(uint32_t, (float)x[0]) & 0x7fffffffu;
    a1 = nan_bits16(raw >> 16) ? 0u : __builtin_bit_cast(uint32_t, (float)x[1]) & 0x7fffffffu;
  }
  uint32_t m = a0 > a1 ? a0 : a1;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, d);
    m = m > o ? m : o;
  }
  const uint32_t floor_bits = __builtin_bit_cast(uint32_t, 1e-4f);
  float s = __builtin_bit_cast(float, m > floor_bits ? m : floor_bits) / 448.0f;
  if (pow2) s = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, s) + 0x007fffffu) & 0x7f800000u);   // (s is a positive normal)

  float lo, hi;
  uint32_t nan;
  if constexpr (BF16) kv8_quot2_bf16(raw, s, lo, hi, nan);
  else kv8_quot2(raw, s, lo, hi, nan);
  const uint32_t codes = ((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(lo, hi, 0, false) & 0xffffu) | nan;
  *reinterpret_cast<uint16_t*>(K8 + prow * 128 + lane * 2) = (uint16_t)codes;
  if (lane == 0) Ks[prow] = s;
}

}  // namespace lc
