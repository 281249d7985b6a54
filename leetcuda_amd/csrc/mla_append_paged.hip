// mla_append_paged.hip — RMSNorm + rotary embedding + append for the paged multi-head latent attention cache (lc_mla_append_paged_f16 / _bf16 /
// _kv8 / _kv8_bf16): the write side of what attn_mla.hip / attn_mla_kv8.hip read.  The outputs of a step's two projections go in
// as they sit in memory — CKVnew [T,512] and KPEnew [T,64] with a row stride each (two pointers into one kv_a_proj_with_mqa output), Qpe [T,H,64]
// with a row and a head stride (a pointer into the q_b_proj output) — and ONE launch leaves
//   - the latent row, normalised (y = x rsqrt(mean(x^2) + eps) gamma in fp32, ONE rounding to the element type), in CKVpool
//     [num_pages, page_size, 512]; KV8: the e4m3fn codes of that ROUNDED row under ckv_scale[0] (kv8_quantize8 / kv8_quantize8_bf16), so that the
//     fp8 pool equals the 16-bit pool quantised afterwards.  gamma == nullptr: no normalisation — a bit copy, or the codes of the row itself
//   - the rotated k_pe row in KPEpool [num_pages, page_size, 64], 16-bit whatever the latent pool holds
//   - the rotated q_pe rows of all H heads in Qpe_out, dense [T,H,64] (may be Qpe itself when Qpe is dense: a row lives in 8 lanes of one wave
//     and every store of a lane depends on its loads — rope_append_paged.hip)
// The rule of a token is rope_append_varlen.hip's, word for word (mla_token_owner below restates its search and clamps; the rotation and the
// codes ARE its functions: rope_rotate8*, rope_partner_chunk, kv8_quantize8*): owner b with cu_q[b] <= t < cu_q[b + 1] by a binary search,
// q0 = clamp(cu_q[b], 0, T), Nq_b = clamp(cu_q[b + 1] - q0, 0, min(max_nq, T - q0)), i = t - q0, position p = L_b - Nq_b + i with
// L_b = clamp(kv_len[b], 0, max_pages page_size); p < 0: a zero row in Qpe_out and no pool write; a page id outside [0, num_pages) drops the two
// pool rows and leaves Qpe_out alone; the cos_sin row read is clamp(p, 0, max_pos - 1); a token nobody owns writes nothing.  rot_dim is the whole 64.
//
// Work split, workgroups of 256, the latent ones first in the 1-D grid:
//   latent   ONE WAVE OWNS ONE TOKEN at a time, tpw consecutive tokens in turn (the host's choice, below).  A 512-wide row is 64 lanes x one
//            16-byte load: one contiguous 1 KiB row per instruction.  The token is wave-uniform (readfirstlane of the wave id), so the search of
//            cu_q, kv_len[b], the page id and the page base are scalar loads and scalar arithmetic.  Sum of squares: 8 lane-local fp32 fmas, then
//            four DPP steps (quad_perm xor 1, xor 2, row_ror 4, row_ror 8) leave every row of 16 lanes its sum and three additions of the four
//            rows' lane 0 (v_readlane) the wave's — one value, the same for every lane.  No LDS, no barrier.  gamma is 8 floats a lane, loaded
//            once per wave.  Stores: 16 bytes a lane, or 8 bytes a lane of codes.  Lanes 0 .. 7 of the same wave rotate and store the token's
//            128-byte k_pe row (their loads are issued in front of the reduction).
//   Q        8 lanes a head row, 32 head rows a workgroup, flattened over (t, h) with h fastest: the 8 table loads of a token's 256-byte cos_sin
//            row are shared by its heads through the caches.  At H = 128 this part is more than 90 % of a step's bytes; every element is read
//            and written once with 16-byte accesses (NeoX: the partner chunk is loaded a second time, from a line the wave fetches anyway).
// Tokens per wave (mla_append_tokens_per_wave, lc_plan.h): 1 up to T = 2048 — a decode step of B tokens spreads over B waves of B / 4
// workgroups — and 4 above it, where gamma's 2 KiB per wave would otherwise be a quarter of the latent traffic again.  Never from device data.
// Plain HIP with builtins; every store is an ordinary vector store.  No scratch, no LDS (isa_audit_mla_append.json).
#pragma once
#include "rope_append_paged.hip"

namespace lc {

constexpr int MLA_APPEND_DC = 512, MLA_APPEND_DR = 64;
constexpr int MLA_APPEND_QROWS = 32;   // head rows of a Q workgroup: 256 lanes / (64 / 8)

// The sequence b that owns token t < T and the token's position p (rope_append_varlen.hip's search and clamps); false: nobody's token
LC_DEVINL bool mla_token_owner(const int* __restrict__ cu_q, const int* __restrict__ kv_len, int B, int T, int max_nq, int ncap, int t, int& b,
                               int& p) {
  int lo = 0, hi = B;
  while (lo < hi) {                             // the first b whose end lies behind t (zero-length sequences are stepped over)
    const int mid = (lo + hi) >> 1;
    if (cu_q[mid + 1] <= t) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= B) return false;                    // t >= cu_q[B]
  b = lo;
  const int q0 = min(max(cu_q[b], 0), T);
  const int c1 = cu_q[b + 1];
  const int nqb = c1 <= q0 ? 0 : min(c1 - q0, min(max_nq, T - q0));
  const int i = t - q0;
  if (i < 0 || i >= nqb) return false;          // outside the sequence under the clamps
  p = min(max(kv_len[b], 0), ncap) - nqb + i;
  return true;
}

// x + (x of the lane DPP control `CTRL` names), all lanes active
template <int CTRL>
LC_DEVINL float mla_dpp_add(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false);
  return x + __builtin_bit_cast(float, y);
}

// The sum of one value per lane over the wave, the SAME bits in every lane (called with all 64 lanes active): butterflies inside a quad, two
// rotations inside a row of 16, then the four rows' lane 0
LC_DEVINL float mla_wave_sum(float x) {
  x = mla_dpp_add<0xB1>(x);    // quad_perm [1,0,3,2]
  x = mla_dpp_add<0x4E>(x);    // quad_perm [2,3,0,1]
  x = mla_dpp_add<0x124>(x);   // row_ror 4
  x = mla_dpp_add<0x128>(x);   // row_ror 8
  const int v = __builtin_bit_cast(int, x);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(v, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(v, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(v, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(v, 48));
  return (r0 + r1) + (r2 + r3);
}

// 8 elements of a row (one 16-byte chunk) as fp32
template <bool BF16>
LC_DEVINL void mla_decode8(u32x4_t raw, float (&x)[8]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t w = raw[d];   // (a copy: __builtin_bit_cast of the vector ELEMENT itself reads element 0 for every d)
    if constexpr (BF16) {
      x[2 * d] = bf16_lo(w);
      x[2 * d + 1] = bf16_hi(w);
    } else {
      const half2_t h = __builtin_bit_cast(half2_t, w);
      x[2 * d] = (float)h[0];
      x[2 * d + 1] = (float)h[1];
    }
  }
}

// ... and back: ONE rounding to the element type (RNE; denormals kept)
template <bool BF16>
LC_DEVINL u32x4_t mla_encode8(const float (&y)[8]) {
  u32x4_t out;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if constexpr (BF16) {
      out[d] = bf16_pack2(y[2 * d], y[2 * d + 1]);
    } else {
      const half2_t h = {(half_t)y[2 * d], (half_t)y[2 * d + 1]};
      out[d] = __builtin_bit_cast(uint32_t, h);
    }
  }
  return out;
}

template <bool BF16, bool INTERLEAVED>
LC_DEVINL u32x4_t mla_rotate8(u32x4_t own, u32x4_t other, const float* __restrict__ cs, unsigned c) {
  if constexpr (BF16) return rope_rotate8_bf16<INTERLEAVED>(own, other, cs, c, MLA_APPEND_DR);
  else return rope_rotate8<INTERLEAVED>(own, other, cs, c, MLA_APPEND_DR);
}

// grid: nlat = ceil(T / (4 tpw)) latent workgroups, then ceil(T H / 32) Q workgroups; lps = log2(page_size)
template <bool KV8, bool BF16, bool INTERLEAVED>
LC_DEVINL void mla_append_paged_body(const half_t* __restrict__ CKVnew, const half_t* __restrict__ KPEnew, const half_t* Qpe, half_t* Qpe_out,
                                     void* __restrict__ CKVpool, half_t* __restrict__ KPEpool, const float* __restrict__ gamma,
                                     const float* __restrict__ cos_sin, const int* __restrict__ cu_q, const int* __restrict__ block_table,
                                     const int* __restrict__ kv_len, const float* __restrict__ ckv_scale, int B, int H, int T, int max_nq,
                                     int num_pages, int lps, int max_pages, int max_pos, float eps, long long ckv_row_stride,
                                     long long kpe_row_stride, long long q_row_stride, long long q_head_stride, int tpw, unsigned nlat) {
  constexpr int DC = MLA_APPEND_DC, DR = MLA_APPEND_DR;
  const unsigned blk = __builtin_amdgcn_workgroup_id_x(), tid = __builtin_amdgcn_workitem_id_x();
  const int ncap = max_pages << lps;
  if (blk >= nlat) {
    // ---- Q: head row r = t H + h, 8 lanes a row
    const unsigned r = (blk - nlat) * MLA_APPEND_QROWS + tid / 8, c = tid % 8;
    const unsigned t = r / (unsigned)H, h = r - t * (unsigned)H;
    if (t >= (unsigned)T) return;
    int b, p;
    if (!mla_token_owner(cu_q, kv_len, B, T, max_nq, ncap, (int)t, b, p)) return;
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(Qpe_out + (size_t)r * DR + c * 8);
    if (p < 0) {                                                  // more tokens than keys: no visible key, a defined value
      *dst = u32x4_t{0u, 0u, 0u, 0u};
      return;
    }
    const size_t row = (size_t)t * (size_t)q_row_stride + (size_t)h * (size_t)q_head_stride;
    const float* cs = cos_sin + (size_t)min(p, max_pos - 1) * DR;   // the row read is clamped: nothing outside the table
    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(Qpe + row + c * 8);
    const u32x4_t qp = INTERLEAVED ? q : *reinterpret_cast<const u32x4_t*>(Qpe + row + rope_partner_chunk<INTERLEAVED>(c, DR) * 8);
    *dst = mla_rotate8<BF16, INTERLEAVED>(q, qp, cs, c);
    return;
  }
  // ---- latent: wave w of the grid walks tokens w tpw .. w tpw + tpw - 1; everything but the lane's chunk is wave-uniform
  const unsigned lane = tid & 63u;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blk * 4u + (tid >> 6)));
  const int t0 = wave * tpw, t1 = min(t0 + tpw, T);   // (nlat 4 tpw < 2^31 + 4 tpw: the host bounds T + 4 tpw)
  if (t0 >= t1) return;
  float g[8];
  if (gamma) {
    const f32x4_t g0 = rope_table4(gamma + lane * 8), g1 = rope_table4(gamma + lane * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g[e] = g0[e];
      g[4 + e] = g1[e];
    }
  }
  float scale = 1.0f;
  if constexpr (KV8) scale = ckv_scale ? ckv_scale[0] : 1.0f;
  for (int t = t0; t < t1; ++t) {
    int b, p;
    if (!mla_token_owner(cu_q, kv_len, B, T, max_nq, ncap, t, b, p)) continue;
    if (p < 0) continue;
    const int pid = block_table[(size_t)b * max_pages + (p >> lps)];   // p < L <= ncap: inside the table row
    if ((unsigned)pid >= (unsigned)num_pages) continue;          // a bad page id drops the token's two pool rows
    const size_t prow = ((size_t)pid << lps) + (unsigned)(p & ((1 << lps) - 1));   // the token's row in both pools
    const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(CKVnew + (size_t)t * (size_t)ckv_row_stride + lane * 8);
    if (lane < 8) {                                              // the k_pe row: 8 chunks of 16 bytes
      const half_t* src = KPEnew + (size_t)t * (size_t)kpe_row_stride;
      const float* cs = cos_sin + (size_t)min(p, max_pos - 1) * DR;
      const u32x4_t k = *reinterpret_cast<const u32x4_t*>(src + lane * 8);
      const u32x4_t kp = INTERLEAVED ? k : *reinterpret_cast<const u32x4_t*>(src + rope_partner_chunk<INTERLEAVED>(lane, DR) * 8);
      *reinterpret_cast<u32x4_t*>(KPEpool + prow * DR + lane * 8) = mla_rotate8<BF16, INTERLEAVED>(k, kp, cs, lane);
    }
    u32x4_t row16 = raw;
    if (gamma) {                                                 // (uniform: all 64 lanes take the reduction)
      float x[8];
      mla_decode8<BF16>(raw, x);
      float ss = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(x[e], x[e], ss);
      const float rinv = __builtin_amdgcn_rsqf(__builtin_fmaf(mla_wave_sum(ss), 1.0f / DC, eps));
      float y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = (x[e] * rinv) * g[e];
      row16 = mla_encode8<BF16>(y);
    }
    if constexpr (KV8) {                                         // the codes of the row ROUNDED to the element type
      uint8_t* dst = static_cast<uint8_t*>(CKVpool) + prow * DC + lane * 8;
      if constexpr (BF16) *reinterpret_cast<u32x2_t*>(dst) = kv8_quantize8_bf16(row16, scale);
      else *reinterpret_cast<u32x2_t*>(dst) = kv8_quantize8(row16, scale);
    } else {
      *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(CKVpool) + prow * DC + lane * 8) = row16;
    }
  }
}

// The four kernels: the body behind the pool type its flags select; a 16-bit pool kernel takes no scale.
// MlaAppendKernel<KV8, BF16>::kernel<INTERLEAVED>() hands a kernel to the launcher (tu_mla_append.hip)
template <bool KV8, bool BF16>
struct MlaAppendKernel;

#define LC_MLA_APPEND_POOL_false half_t *__restrict__ CKVpool
#define LC_MLA_APPEND_POOL_true uint8_t *__restrict__ CKVpool8, const float *__restrict__ ckv_scale
#define LC_MLA_APPEND_POOL_USE_false CKVpool
#define LC_MLA_APPEND_POOL_USE_true CKVpool8
#define LC_MLA_APPEND_SCALE_USE_false nullptr
#define LC_MLA_APPEND_SCALE_USE_true ckv_scale
#define LC_MLA_APPEND_KERNEL(NAME, KV8_, BF16_)                                                                                                  \
  template <bool INTERLEAVED>                                                                                                                   \
  __global__ __launch_bounds__(256) void NAME(const half_t *__restrict__ CKVnew, const half_t *__restrict__ KPEnew, const half_t *Qpe,          \
                                              half_t *Qpe_out, LC_MLA_APPEND_POOL_##KV8_, half_t *__restrict__ KPEpool,                         \
                                              const float *__restrict__ gamma, const float *__restrict__ cos_sin, const int *__restrict__ cu_q, \
                                              const int *__restrict__ block_table, const int *__restrict__ kv_len, int B, int H, int T,         \
                                              int max_nq, int num_pages, int lps, int max_pages, int max_pos, float eps,                        \
                                              long long ckv_row_stride, long long kpe_row_stride, long long q_row_stride,                       \
                                              long long q_head_stride, int tpw, unsigned nlat) {                                                \
    mla_append_paged_body<KV8_, BF16_, INTERLEAVED>(CKVnew, KPEnew, Qpe, Qpe_out, LC_MLA_APPEND_POOL_USE_##KV8_, KPEpool, gamma, cos_sin, cu_q,  \
                                                    block_table, kv_len, LC_MLA_APPEND_SCALE_USE_##KV8_, B, H, T, max_nq, num_pages, lps,       \
                                                    max_pages, max_pos, eps, ckv_row_stride, kpe_row_stride, q_row_stride, q_head_stride, tpw,  \
                                                    nlat);                                                                                      \
  }                                                                                                                                             \
  template <>                                                                                                                                   \
  struct MlaAppendKernel<KV8_, BF16_> {                                                                                                         \
    template <bool INTERLEAVED>                                                                                                                 \
    static auto kernel() { return NAME<INTERLEAVED>; }                                                                                          \
  };

LC_MLA_APPEND_KERNEL(mla_append_paged_kernel, false, false)
LC_MLA_APPEND_KERNEL(mla_append_paged_bf16_kernel, false, true)
LC_MLA_APPEND_KERNEL(mla_append_paged_kv8_kernel, true, false)
LC_MLA_APPEND_KERNEL(mla_append_paged_kv8_bf16_kernel, true, true)

#undef LC_MLA_APPEND_POOL_false
#undef LC_MLA_APPEND_POOL_true
#undef LC_MLA_APPEND_POOL_USE_false
#undef LC_MLA_APPEND_POOL_USE_true
#undef LC_MLA_APPEND_SCALE_USE_false
#undef LC_MLA_APPEND_SCALE_USE_true
#undef LC_MLA_APPEND_KERNEL

}  // namespace lc
