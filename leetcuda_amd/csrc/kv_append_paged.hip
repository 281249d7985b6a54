// kv_append_paged.hip — the write side of the paged KV cache (lc_kv_append_paged_f16 / lc_kv_append_paged_kv8): the K and V rows
// of the Nq newest tokens of every sequence go into the pools [num_pages, Hkv, page_size, D] through the block table and the kv_len array that
// the decode call of the same step reads next, as fp16 or quantised to OCP e4m3fn on the way.  ONE launch writes K and V.
//   - where a token goes: L = clamp(kv_len[b], 0, max_pages x page_size) is the length AFTER the append (the decode kernels' clamp), token i sits
//     at position p = L - Nq + i — the position the bottom-right causal mask gives query i.  p < 0: not written (left padding).  Page
//     block_table[b][p / page_size], row p % page_size, every K / V head.  A page id outside [0, num_pages) DROPS the token: a read may clamp a
//     bad id, a write to a clamped page would land in another sequence's cache.  Table entries of pages that hold none of the Nq positions are
//     never read.  Two batch entries that name the same page and row: which one lands is unspecified.
//   - mapping: the call is bound by bytes (prefill) or by launch latency (Nq = 1), so all there is to design is full-width accesses.  A lane takes
//     one 16-byte chunk (8 fp16) of a K row AND the same chunk of the V row: two independent dwordx4 loads in flight per lane, one kv_len / table
//     read and one address computation for both.  D / 8 lanes cover a row, 2048 / D consecutive tokens of one (batch entry, K / V head) a
//     workgroup of 256: loads are one contiguous 4 KiB run per workgroup and tensor, a row's stores one 2 D-byte (fp16: dwordx4) or D-byte (fp8:
//     dwordx2 after four packed conversions) run, the rows of a page contiguous.  Batch entry and head are uniform in a workgroup: the
//     two integer divisions that find them, kv_len[b] and the scales are scalar work; a lane has shifts and masks only.
//   - the page base is 64 bit (a pool may exceed 4 GiB), the offset inside a (page, head) run 32 bit (the host bounds the run below 2 GiB).
//   - fp8: code = e4m3fn_rne(clamp(fp32(x) / s, -448, 448)), the quotient the correctly rounded IEEE division (what a reader that multiplies by
//     s expects, and what tests/decode_lib.quantize computes — not a multiplication by a rounded reciprocal).  The clamp is done in fp32 in
//     front of the conversion, so nothing depends on what v_cvt_pk_fp8_f32 makes of |x| > 448; +-inf gives +-448, -0 gives 0x80.  A NaN is
//     found on the BITS of the input (and of the quotient): the units are built with -fno-honor-nans, under which a float compare is no route
//     for a NaN, and v_med3_f32 does not propagate one.  Its code gets 0x7F or-ed in.
// Plain HIP with builtins; every store is an ordinary vector store.
#pragma once
#include "lc_common.h"

namespace lc {

LC_DEVINL bool nan_bits16(uint32_t h) { return (h & 0x7fffu) > 0x7c00u; }
LC_DEVINL bool nan_bits32(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7fffffffu) > 0x7f800000u; }

// the two fp16 of one dword -> fp32(x) / s clamped to +-448; nan: or-mask of the two result bytes (0x7f per NaN)
LC_DEVINL void kv8_quot2(uint32_t w, float s, float& lo, float& hi, uint32_t& nan) {
  const half2_t h = __builtin_bit_cast(half2_t, w);
  const float ql = (float)h[0] / s, qh = (float)h[1] / s;
  nan = ((nan_bits16(w) || nan_bits32(ql)) ? 0x7fu : 0u) | ((nan_bits16(w >> 16) || nan_bits32(qh)) ? 0x7f00u : 0u);
  lo = __builtin_amdgcn_fmed3f(ql, -448.0f, 448.0f);
  hi = __builtin_amdgcn_fmed3f(qh, -448.0f, 448.0f);
}

// 8 fp16 (one 16-byte chunk) -> 8 e4m3fn bytes under scale s
LC_DEVINL u32x2_t kv8_quantize8(u32x4_t raw, float s) {
  u32x2_t out;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float a, b, c, d;
    uint32_t n0, n1;
    kv8_quot2(raw[2 * j], s, a, b, n0);
    kv8_quot2(raw[2 * j + 1], s, c, d, n1);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);   // bytes 0, 1
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);        // bytes 2, 3
    out[j] = (uint32_t)w | n0 | (n1 << 16);
  }
  return out;
}

// The bfloat16 flavours of the two functions above (rope_append_varlen.hip): a bf16 element IS the upper half of its fp32
// value, so the decode is a shift; the quotient, the clamp, the conversion and the NaN rule are the same, the NaN test on the bf16 bits
LC_DEVINL bool nan_bits_bf16(uint32_t h) { return (h & 0x7fffu) > 0x7f80u; }
LC_DEVINL float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }           // element 0 of a dword of two bf16
LC_DEVINL float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }   // element 1
// two fp32 -> one dword of two bf16 (RNE), element 0 in the low half
LC_DEVINL uint32_t bf16_pack2(float lo, float hi) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}

// kv8_quot2 for the two bf16 of one dword
LC_DEVINL void kv8_quot2_bf16(uint32_t w, float s, float& lo, float& hi, uint32_t& nan) {
  const float ql = bf16_lo(w) / s, qh = bf16_hi(w) / s;
  nan = ((nan_bits_bf16(w) || nan_bits32(ql)) ? 0x7fu : 0u) | ((nan_bits_bf16(w >> 16) || nan_bits32(qh)) ? 0x7f00u : 0u);
  lo = __builtin_amdgcn_fmed3f(ql, -448.0f, 448.0f);
  hi = __builtin_amdgcn_fmed3f(qh, -448.0f, 448.0f);
}

// 8 bf16 (one 16-byte chunk) -> 8 e4m3fn bytes under scale s
LC_DEVINL u32x2_t kv8_quantize8_bf16(u32x4_t raw, float s) {
  u32x2_t out;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float a, b, c, d;
    uint32_t n0, n1;
    kv8_quot2_bf16(raw[2 * j], s, a, b, n0);
    kv8_quot2_bf16(raw[2 * j + 1], s, c, d, n1);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);   // bytes 0, 1
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);        // bytes 2, 3
    out[j] = (uint32_t)w | n0 | (n1 << 16);
  }
  return out;
}

template <int D, bool KV8>
LC_DEVINL void kv_append_paged_body(const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew, void* __restrict__ Kpool, void* __restrict__ Vpool,
                                    const int* __restrict__ block_table, const int* __restrict__ kv_len, const float* __restrict__ k_scale,
                                    const float* __restrict__ v_scale, int Hkv, int Nq, int num_pages, int lps, int max_pages, int bph) {
  constexpr int LPR = D / 8, TPB = 256 / LPR;   // lanes per row, tokens per workgroup
  // uniform: the (batch entry, K / V head) and the token block of this workgroup (the id builtins: an SGPR the compiler KNOWS to be uniform, so
  // the two divisions and everything derived from them are scalar work)
  const unsigned blk = __builtin_amdgcn_workgroup_id_x(), tid = __builtin_amdgcn_workitem_id_x();
  const unsigned bh = blk / (unsigned)bph, tb = blk - bh * (unsigned)bph;
  const unsigned b = bh / (unsigned)Hkv, h = bh - b * (unsigned)Hkv;
  const unsigned i = tb * TPB + tid / LPR, c = tid % LPR;
  if (i >= (unsigned)Nq) return;
  const int ncap = max_pages << lps;
  const int L = min(max(kv_len[b], 0), ncap);
  const int p = L - Nq + (int)i;
  if (p < 0) return;                                             // left padding
  const int pid = block_table[(size_t)b * max_pages + (p >> lps)];   // p < L <= ncap: inside the table row
  if ((unsigned)pid >= (unsigned)num_pages) return;             // a bad page id drops the token
  const size_t src = ((size_t)bh * (unsigned)Nq + i) * D + c * 8;
  const u32x4_t k = *reinterpret_cast<const u32x4_t*>(Knew + src);
  const u32x4_t v = *reinterpret_cast<const u32x4_t*>(Vnew + src);
  const size_t run = ((size_t)pid * (unsigned)Hkv + h) << lps;   // first row of the (page, head) run
  const unsigned off = (unsigned)(p & ((1 << lps) - 1)) * D + c * 8;   // elements inside the run
  if constexpr (KV8) {
    const float ks = k_scale ? k_scale[h] : 1.0f, vs = v_scale ? v_scale[h] : 1.0f;
    *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Kpool) + run * D + off) = kv8_quantize8(k, ks);
    *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Vpool) + run * D + off) = kv8_quantize8(v, vs);
  } else {
    *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(Kpool) + run * D + off) = k;
    *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(Vpool) + run * D + off) = v;
  }
}

// grid: B x Hkv x bph workgroups of 256, bph = ceil(Nq / (2048 / D)); lps = log2(page_size)
template <int D>
__global__ __launch_bounds__(256) void kv_append_paged_kernel(const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew, half_t* __restrict__ Kpool,
                                                              half_t* __restrict__ Vpool, const int* __restrict__ block_table,
                                                              const int* __restrict__ kv_len, int Hkv, int Nq, int num_pages, int lps, int max_pages,
                                                              int bph) {
  kv_append_paged_body<D, false>(Knew, Vnew, Kpool, Vpool, block_table, kv_len, nullptr, nullptr, Hkv, Nq, num_pages, lps, max_pages, bph);
}

template <int D>
__global__ __launch_bounds__(256) void kv_append_paged_kv8_kernel(const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew,
                                                                  uint8_t* __restrict__ Kpool8, uint8_t* __restrict__ Vpool8,
                                                                  const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                                  const float* __restrict__ k_scale, const float* __restrict__ v_scale, int Hkv, int Nq,
                                                                  int num_pages, int lps, int max_pages, int bph) {
  kv_append_paged_body<D, true>(Knew, Vnew, Kpool8, Vpool8, block_table, kv_len, k_scale, v_scale, Hkv, Nq, num_pages, lps, max_pages, bph);
}

}  // namespace lc
