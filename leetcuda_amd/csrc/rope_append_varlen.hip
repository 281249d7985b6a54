// rope_append_varlen.hip — rotary embedding + append for a ragged batch (lc_rope_append_varlen_f16 / _kv8): the write side of
// the step that attn_varlen.hip reads.  The rule of a token is rope_append_paged.hip's, word for word — rope_rotate8 and kv8_quantize8
// themselves — and what changes is how a row finds its sequence:
//   - sources are token-major with a row stride each: element (t, h, d) of Q at Q[t q_row_stride + h D + d], of Knew / Vnew at
//     ptr[t kv_row_stride + h D + d] (three pointers into one projection output [T, (H + 2 Hkv) D], or dense [T,H,D] / [T,Hkv,D]); Qout is dense
//     [T,H,D], the layout attn_varlen.hip reads, and may be Q itself when q_row_stride = H D (a row lives in one wave: rope_append_paged.hip)
//   - the grid is over GLOBAL token blocks: ceil(T / (2048 / D)) x (Hkv + H) workgroups, the K/V ones first.  It does not grow with B x max_nq.
//     A block may straddle sequences, so b, L_b and the page are per ROW: each row finds the sequence b with cu_q[b] <= t < cu_q[b + 1] by a
//     binary search of cu_q — at most log2(B + 1) + 1 loads of an array that stays in the caches — and then applies attn_varlen.hip's clamps:
//     q0 = clamp(cu_q[b], 0, T), Nq_b = clamp(cu_q[b + 1] - q0, 0, min(max_nq, T - q0)), i = t - q0, position p = L_b - Nq_b + i
//   - a token no sequence owns (t >= cu_q[B], or i outside [0, Nq_b) under the clamps) writes nothing, in the pools or in Qout
// Only t < T is ever used as a row: no value in cu_q takes a load or a store outside the T rows.
//
// The family is ONE body and three flags, every value of which exists.  A kernel's name states them:
//   rope_append_varlen_ [pos_] [kv8_] [bf16_] kernel<D, INTERLEAVED>
// KV8 (§4.3l): the pools are e4m3 bytes, and k_scale, v_scale follow kv_len; a 16-bit pool kernel takes neither.
// BF16 (lc_rope_append_varlen_*bf16; §4.3m): sources, Qout and 16-bit pools are bfloat16.  The body — the lane map, the binary search of cu_q, the
//   clamps and the drop rules — is the same, with rope_rotate8_bf16 (rope_append_paged.hip) and kv8_quantize8_bf16 (kv_append_paged.hip) in place
//   of the fp16 functions:
//   - a bf16 element IS the upper half of its fp32 value: the decode is a shift, exact, denormals included
//   - the arithmetic is rope_fma, the fp16 kernels' one rounded product and one fma in fp32, then ONE rounding to bf16 (RNE, v_cvt_pk_bf16_f32;
//     bf16 denormals are fp32 denormals and are kept).  Elements at or behind rot_dim, and all of V, are copied bit for bit
//   - fp8 pools: code = e4m3fn_rne(clamp(fp32(x) / s, -448, 448)) with the true division, taken of the rotated row ROUNDED TO bf16 first, so
//     that the pool equals what a bf16 pool quantised afterwards would hold.  A NaN is found on the bf16 bits ((h & 0x7fff) > 0x7f80) and on the
//     quotient; its code gets 0x7F or-ed in.  +-inf gives +-448
//   The fp16 flavours (rope_rotate8, kv8_quot2, kv8_quantize8) stay what they are; the bf16 ones are defined next to them.
// POS (lc_rope_append_varlen_pos_*; §4.3o): the rotary position of every token is stated by the caller, pos_ids (device int32[T]) behind
//   kv_row_stride.  The nodes of a draft tree sit in neighbouring cache slots, but a node's rotary position is prefix length + depth: siblings
//   share one.  It changes ONE thing: the cos_sin row of token t is clamp(pos_ids[t], 0, max_pos - 1) in place of clamp(p, 0, max_pos - 1).  The
//   cache slot p = L_b - Nq_b + i, the p < 0 rule, dropped tokens, quantisation, strides and in-place Q are the twin's; pos_ids[t] = p for every
//   token gives the twin's bytes.  pos_ids is read only for a token that a sequence owns.
#pragma once
#include "rope_append_paged.hip"

namespace lc {

template <int D, bool INTERLEAVED, bool KV8, bool BF16 = false, bool POS = false>
LC_DEVINL void rope_append_varlen_body(const half_t* Q, const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew, half_t* Qout,
                                       void* __restrict__ Kpool, void* __restrict__ Vpool, const float* __restrict__ cos_sin,
                                       const int* __restrict__ cu_q, const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                       const float* __restrict__ k_scale, const float* __restrict__ v_scale, int B, int H, int Hkv, int T,
                                       int max_nq, int num_pages, int lps, int max_pages, int nblk, int rot_dim, int max_pos,
                                       long long q_row_stride, long long kv_row_stride, const int* __restrict__ pos_ids = nullptr) {
  constexpr int LPR = D / 8, TPB = 256 / LPR;   // lanes per row, tokens per workgroup
  // uniform: the role, the head and the token block of this workgroup
  const unsigned blk0 = __builtin_amdgcn_workgroup_id_x(), tid = __builtin_amdgcn_workitem_id_x();
  const unsigned nkv = (unsigned)Hkv * (unsigned)nblk;
  const bool isq = blk0 >= nkv;                 // the Q workgroups follow the Hkv x nblk K/V workgroups
  const unsigned blk = isq ? blk0 - nkv : blk0;
  const unsigned h = blk / (unsigned)nblk, tb = blk - h * (unsigned)nblk;
  const unsigned r = tid / LPR, c = tid % LPR, t = tb * TPB + r;
  if (t >= (unsigned)T) return;
  // the sequence of token t: the first b whose end lies behind t (zero-length sequences are stepped over)
  int lo = 0, hi = B;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cu_q[mid + 1] <= (int)t) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= B) return;                          // t >= cu_q[B]: nobody's token
  const int b = lo;
  const int q0 = min(max(cu_q[b], 0), T);
  const int c1 = cu_q[b + 1];
  const int nqb = c1 <= q0 ? 0 : min(c1 - q0, min(max_nq, T - q0));
  const int i = (int)t - q0;
  if (i < 0 || i >= nqb) return;                // outside the sequence under the clamps (a cu_q that is not monotone, Nq_b > max_nq)
  const int ncap = max_pages << lps;
  const int L = min(max(kv_len[b], 0), ncap);
  const int p = L - nqb + i;
  const size_t rowq = (size_t)t * (size_t)q_row_stride + (size_t)h * D, rowkv = (size_t)t * (size_t)kv_row_stride + (size_t)h * D;
  const unsigned cp = rope_partner_chunk<INTERLEAVED>(c, rot_dim);   // the partner chunk of the same row
  int rp = p;   // the rotary position (POS: the caller's, read only for an owned token t < T)
  if constexpr (POS) rp = pos_ids[t];
  const float* cs = cos_sin + (size_t)min(max(rp, 0), max_pos - 1) * (unsigned)rot_dim;   // the row read is clamped: nothing outside the table
  if (isq) {
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(Qout + ((size_t)t * (unsigned)H + h) * D + c * 8);
    if (p < 0) {                                                 // more tokens than keys: no visible key, a defined value
      *dst = u32x4_t{0u, 0u, 0u, 0u};
      return;
    }
    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(Q + rowq + c * 8);
    const u32x4_t qp = INTERLEAVED ? q : *reinterpret_cast<const u32x4_t*>(Q + rowq + cp * 8);
    if constexpr (BF16) *dst = rope_rotate8_bf16<INTERLEAVED>(q, qp, cs, c, rot_dim);
    else *dst = rope_rotate8<INTERLEAVED>(q, qp, cs, c, rot_dim);
    return;
  }
  if (p < 0) return;
  const int pid = block_table[(size_t)b * max_pages + (p >> lps)];   // p < L <= ncap: inside the table row
  if ((unsigned)pid >= (unsigned)num_pages) return;             // a bad page id drops the token
  const u32x4_t k = *reinterpret_cast<const u32x4_t*>(Knew + rowkv + c * 8);
  const u32x4_t kp = INTERLEAVED ? k : *reinterpret_cast<const u32x4_t*>(Knew + rowkv + cp * 8);
  const u32x4_t v = *reinterpret_cast<const u32x4_t*>(Vnew + rowkv + c * 8);
  u32x4_t kr;
  if constexpr (BF16) kr = rope_rotate8_bf16<INTERLEAVED>(k, kp, cs, c, rot_dim);
  else kr = rope_rotate8<INTERLEAVED>(k, kp, cs, c, rot_dim);
  const size_t run = ((size_t)pid * (unsigned)Hkv + h) << lps;   // first row of the (page, head) run
  const unsigned off = (unsigned)(p & ((1 << lps) - 1)) * D + c * 8;   // elements inside the run
  if constexpr (KV8) {
    const float ks = k_scale ? k_scale[h] : 1.0f, vs = v_scale ? v_scale[h] : 1.0f;
    if constexpr (BF16) {   // the codes of the row ROUNDED to bf16
      *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Kpool) + run * D + off) = kv8_quantize8_bf16(kr, ks);
      *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Vpool) + run * D + off) = kv8_quantize8_bf16(v, vs);
    } else {
      *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Kpool) + run * D + off) = kv8_quantize8(kr, ks);   // the codes of the row ROUNDED to fp16
      *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Vpool) + run * D + off) = kv8_quantize8(v, vs);
    }
  } else {
    *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(Kpool) + run * D + off) = kr;
    *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(Vpool) + run * D + off) = v;
  }
}

// The eight kernels: the body behind the argument list its flags select.  grid: nblk x (Hkv + H) workgroups of 256, nblk = ceil(T / (2048 / D)),
// the first Hkv x nblk of them K/V; lps = log2(page_size).  RopeVarlenKernel<KV8, BF16, POS>::kernel<D, INTERLEAVED>() hands a kernel to the
// launcher (tu_rope_append_varlen_impl.h), so a launcher cannot name a kernel of other flags
template <bool KV8, bool BF16, bool POS>
struct RopeVarlenKernel;

#define LC_ROPE_VARLEN_POOLS_false half_t *__restrict__ Kpool, half_t *__restrict__ Vpool
#define LC_ROPE_VARLEN_POOLS_true uint8_t *__restrict__ Kpool8, uint8_t *__restrict__ Vpool8
#define LC_ROPE_VARLEN_POOLS_USE_false Kpool, Vpool
#define LC_ROPE_VARLEN_POOLS_USE_true Kpool8, Vpool8
#define LC_ROPE_VARLEN_SCALES_false
#define LC_ROPE_VARLEN_SCALES_true const float *__restrict__ k_scale, const float *__restrict__ v_scale,
#define LC_ROPE_VARLEN_SCALES_USE_false nullptr, nullptr
#define LC_ROPE_VARLEN_SCALES_USE_true k_scale, v_scale
#define LC_ROPE_VARLEN_POS_false
#define LC_ROPE_VARLEN_POS_true , const int *__restrict__ pos_ids
#define LC_ROPE_VARLEN_POS_USE_false
#define LC_ROPE_VARLEN_POS_USE_true , pos_ids
#define LC_ROPE_VARLEN_KERNEL(NAME, KV8_, BF16_, POS_)                                                                                          \
  template <int D, bool INTERLEAVED>                                                                                                           \
  __global__ __launch_bounds__(256) void NAME(const half_t *Q, const half_t *__restrict__ Knew, const half_t *__restrict__ Vnew, half_t *Qout, \
                                              LC_ROPE_VARLEN_POOLS_##KV8_, const float *__restrict__ cos_sin, const int *__restrict__ cu_q,    \
                                              const int *__restrict__ block_table, const int *__restrict__ kv_len, LC_ROPE_VARLEN_SCALES_##KV8_ \
                                              int B, int H, int Hkv, int T, int max_nq, int num_pages, int lps, int max_pages, int nblk,       \
                                              int rot_dim, int max_pos, long long q_row_stride,                                                \
                                              long long kv_row_stride LC_ROPE_VARLEN_POS_##POS_) {                                             \
    rope_append_varlen_body<D, INTERLEAVED, KV8_, BF16_, POS_>(Q, Knew, Vnew, Qout, LC_ROPE_VARLEN_POOLS_USE_##KV8_, cos_sin, cu_q, block_table, \
                                                               kv_len, LC_ROPE_VARLEN_SCALES_USE_##KV8_, B, H, Hkv, T, max_nq, num_pages, lps, \
                                                               max_pages, nblk, rot_dim, max_pos, q_row_stride,                                \
                                                               kv_row_stride LC_ROPE_VARLEN_POS_USE_##POS_);                                   \
  }                                                                                                                                            \
  template <>                                                                                                                                  \
  struct RopeVarlenKernel<KV8_, BF16_, POS_> {                                                                                                 \
    template <int D, bool INTERLEAVED>                                                                                                         \
    static auto kernel() { return NAME<D, INTERLEAVED>; }                                                                                      \
  };

LC_ROPE_VARLEN_KERNEL(rope_append_varlen_kernel, false, false, false)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_kv8_kernel, true, false, false)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_bf16_kernel, false, true, false)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_kv8_bf16_kernel, true, true, false)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_pos_kernel, false, false, true)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_pos_kv8_kernel, true, false, true)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_pos_bf16_kernel, false, true, true)
LC_ROPE_VARLEN_KERNEL(rope_append_varlen_pos_kv8_bf16_kernel, true, true, true)

#undef LC_ROPE_VARLEN_POOLS_false
#undef LC_ROPE_VARLEN_POOLS_true
#undef LC_ROPE_VARLEN_POOLS_USE_false
#undef LC_ROPE_VARLEN_POOLS_USE_true
#undef LC_ROPE_VARLEN_SCALES_false
#undef LC_ROPE_VARLEN_SCALES_true
#undef LC_ROPE_VARLEN_SCALES_USE_false
#undef LC_ROPE_VARLEN_SCALES_USE_true
#undef LC_ROPE_VARLEN_POS_false
#undef LC_ROPE_VARLEN_POS_true
#undef LC_ROPE_VARLEN_POS_USE_false
#undef LC_ROPE_VARLEN_POS_USE_true
#undef LC_ROPE_VARLEN_KERNEL

}  // namespace lc
