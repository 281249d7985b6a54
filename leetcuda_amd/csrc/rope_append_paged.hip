// rope_append_paged.hip — rotary embedding fused with the append to the paged KV cache (lc_rope_append_paged_f16 / lc_rope_append_paged_kv8;
// DESIGN.md §4.3j): the projection GEMM's output goes in; rotated Q in the attention calls' layout [B,H,Nq,D] and rotated (fp8: quantised) K plus
// unrotated V in the pools come out.  ONE launch does Q, K and V.
//   - where a token goes is kv_append_paged.hip's rule, word for word: L = clamp(kv_len[b], 0, max_pages x page_size) is the length AFTER the
//     append, token i has position p = L - Nq + i; p < 0 is left padding (no pool write, a ZERO row in Qout); a page id outside [0, num_pages)
//     drops the token's K and V rows and leaves Qout alone.  V is copied (fp8: quantised) exactly as the append kernel does it.
//   - rotation of a Q or K row at position p: row t = min(p, max_pos - 1) of cos_sin (fp32 [max_pos, rot_dim]: rot_dim / 2 cosines, then
//     rot_dim / 2 sines; the caller owns the angles, there is no trigonometry here).  Pair j is elements (j, j + rot_dim / 2) (NeoX, the default)
//     or (2j, 2j + 1) (INTERLEAVED, GPT-J): x1' = x1 c - x2 s, x2' = x2 c + x1 s, fp16 -> fp32, fp32 arithmetic in ONE stated form (a rounded
//     product, then one fma: rope_rotate8, which serves Q and K alike so that the two cannot be contracted differently), one rounding to fp16
//     (RNE; fp16 denormals kept both ways).  Elements rot_dim .. D - 1 are copied bit for bit.
//   - mapping: the append kernel's, extended.  A lane owns one 16-byte chunk (8 fp16) of a row, D / 8 lanes a row, 2048 / D consecutive tokens of
//     one (batch entry, head) a workgroup of 256.  The 1-D grid holds B x Hkv x bph K/V workgroups (a lane rotates its K chunk and moves the same
//     chunk of V), then B x H x bph Q workgroups.  Role, batch entry, head, kv_len[b] and the scales are uniform in a workgroup: the divisions
//     that find them are scalar work on the workgroup id.
//   - the NeoX partner chunk is rot_dim / 16 lanes away in the same row: it is LOADED A SECOND TIME (one more dwordx4 load of a 128-byte line the
//     wave fetches anyway) instead of exchanged through registers — rot_dim / 16 need not be a power of two (rot_dim = 48, 96), so the exchange
//     would be four ds_bpermute per chunk plus their address; DESIGN.md §4.3j.  Interleaved pairs live inside the lane's chunk.
//   - sources: dense [B,H,Nq,D] / [B,Hkv,Nq,D] (src_row_stride = 0), or LC_ROPE_PACKED_SRC: element (b, i, h, d) at
//     ptr[(b Nq + i) src_row_stride + h D + d], the three pointers into one token-major projection output.  A run-time argument: the two
//     layouts differ in one uniform base and one uniform token stride.  64-bit bases, as the page base.
//   - in place (Qout == Q, dense): a row lives in ONE wave (D / 8 <= 16 lanes), and every store of a lane is data-dependent on its loads, own
//     chunk and partner chunk: the wave's s_waitcnt in front of the arithmetic retires the loads of ALL its lanes before any lane stores.
//     Load-then-store program order is all that is needed; Q and Qout are therefore NOT __restrict__.
// Plain HIP with builtins; every store is an ordinary vector store.  kv_append_paged.hip is included for kv8_quantize8 only.
#pragma once
#include "kv_append_paged.hip"

namespace lc {

LC_DEVINL f32x4_t rope_table4(const float* __restrict__ p) {   // the table is aligned as floats are, no more
  f32x4_t v;
  __builtin_memcpy(&v, p, sizeof(v));
  return v;
}

// x c + y s as ONE rounded product and ONE fma (callers pass -s for the x1 row): the only arithmetic of the unit
LC_DEVINL float rope_fma(float x, float c, float y, float s) {
  const float t = y * s;
  return __builtin_fmaf(x, c, t);
}

// The lane's chunk `own` (elements 8c .. 8c + 7 of a row) rotated by table row cs; other: NeoX, the partner chunk (rot_dim / 2 elements away);
// interleaved: unused.  A chunk at or behind rot_dim comes back bit for bit (its table index is clamped to 0: nothing is read past the row).
template <bool INTERLEAVED>
LC_DEVINL u32x4_t rope_rotate8(u32x4_t own, u32x4_t other, const float* __restrict__ cs, unsigned c, int rot_dim) {
  const unsigned rc = (unsigned)rot_dim >> 3, half = (unsigned)rot_dim >> 1;
  const bool rot = c < rc;
  const half8_t x = __builtin_bit_cast(half8_t, own);
  half8_t out;
  if constexpr (INTERLEAVED) {
    const unsigned j = rot ? c * 4 : 0;                 // pairs 4c .. 4c + 3
    const f32x4_t co = rope_table4(cs + j), si = rope_table4(cs + half + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x1 = (float)x[2 * e], x2 = (float)x[2 * e + 1];
      out[2 * e] = (half_t)rope_fma(x1, co[e], x2, -si[e]);
      out[2 * e + 1] = (half_t)rope_fma(x2, co[e], x1, si[e]);
    }
  } else {
    const unsigned hc = rc >> 1;
    const bool second = c >= hc;                        // the lane holds x2 of pairs 8 (c - hc) ..: x2' = x2 c + x1 s
    const unsigned j = rot ? (second ? c - hc : c) * 8 : 0;
    const half8_t y = __builtin_bit_cast(half8_t, other);
    const f32x4_t c0 = rope_table4(cs + j), c1 = rope_table4(cs + j + 4), s0 = rope_table4(cs + half + j), s1 = rope_table4(cs + half + j + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float co = e < 4 ? c0[e & 3] : c1[e & 3], si = e < 4 ? s0[e & 3] : s1[e & 3];
      out[e] = (half_t)rope_fma((float)x[e], co, (float)y[e], second ? si : -si);
    }
  }
  return rot ? __builtin_bit_cast(u32x4_t, out) : own;
}

// rope_rotate8 on a chunk of 8 bf16: the same table indices, the same rope_fma, one rounding to bf16
template <bool INTERLEAVED>
LC_DEVINL u32x4_t rope_rotate8_bf16(u32x4_t own, u32x4_t other, const float* __restrict__ cs, unsigned c, int rot_dim) {
  const unsigned rc = (unsigned)rot_dim >> 3, half = (unsigned)rot_dim >> 1;
  const bool rot = c < rc;
  u32x4_t out;
  if constexpr (INTERLEAVED) {
    const unsigned j = rot ? c * 4 : 0;                 // pairs 4c .. 4c + 3: one dword each
    const f32x4_t co = rope_table4(cs + j), si = rope_table4(cs + half + j);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x1 = bf16_lo(own[e]), x2 = bf16_hi(own[e]);
      out[e] = bf16_pack2(rope_fma(x1, co[e], x2, -si[e]), rope_fma(x2, co[e], x1, si[e]));
    }
  } else {
    const unsigned hc = rc >> 1;
    const bool second = c >= hc;                        // the lane holds x2 of pairs 8 (c - hc) ..: x2' = x2 c + x1 s
    const unsigned j = rot ? (second ? c - hc : c) * 8 : 0;
    const f32x4_t c0 = rope_table4(cs + j), c1 = rope_table4(cs + j + 4), s0 = rope_table4(cs + half + j), s1 = rope_table4(cs + half + j + 4);
#pragma unroll
    for (int d = 0; d < 4; ++d) {                       // dword d: elements 2d, 2d + 1
      const float cl = d < 2 ? c0[2 * d] : c1[2 * d - 4], ch = d < 2 ? c0[2 * d + 1] : c1[2 * d - 3];
      const float sl = d < 2 ? s0[2 * d] : s1[2 * d - 4], sh = d < 2 ? s0[2 * d + 1] : s1[2 * d - 3];
      out[d] = bf16_pack2(rope_fma(bf16_lo(own[d]), cl, bf16_lo(other[d]), second ? sl : -sl),
                          rope_fma(bf16_hi(own[d]), ch, bf16_hi(other[d]), second ? sh : -sh));
    }
  }
  return rot ? out : own;
}

// the chunk a NeoX lane needs besides its own: rot_dim / 16 chunks up or down inside the rotated part, itself behind it
template <bool INTERLEAVED>
LC_DEVINL unsigned rope_partner_chunk(unsigned c, int rot_dim) {
  if constexpr (INTERLEAVED) return c;
  const unsigned rc = (unsigned)rot_dim >> 3, hc = rc >> 1;
  return c >= rc ? c : c >= hc ? c - hc : c + hc;
}

template <int D, bool INTERLEAVED, bool KV8>
LC_DEVINL void rope_append_paged_body(const half_t* Q, const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew, half_t* Qout,
                                      void* __restrict__ Kpool, void* __restrict__ Vpool, const float* __restrict__ cos_sin,
                                      const int* __restrict__ block_table, const int* __restrict__ kv_len, const float* __restrict__ k_scale,
                                      const float* __restrict__ v_scale, int H, int Hkv, int Nq, int num_pages, int lps, int max_pages, int bph,
                                      int rot_dim, int max_pos, long long src_row_stride, unsigned nkv) {
  constexpr int LPR = D / 8, TPB = 256 / LPR;   // lanes per row, tokens per workgroup
  // uniform: the role, the (batch entry, head) and the token block of this workgroup (the id builtin: an SGPR the compiler KNOWS to be uniform)
  const unsigned blk0 = __builtin_amdgcn_workgroup_id_x(), tid = __builtin_amdgcn_workitem_id_x();
  const bool isq = blk0 >= nkv;                 // the Q workgroups follow the nkv = B x Hkv x bph K/V workgroups
  const unsigned blk = isq ? blk0 - nkv : blk0, heads = isq ? (unsigned)H : (unsigned)Hkv;
  const unsigned bh = blk / (unsigned)bph, tb = blk - bh * (unsigned)bph;
  const unsigned b = bh / heads, h = bh - b * heads;
  const unsigned r = tid / LPR, c = tid % LPR, i = tb * TPB + r;
  if (i >= (unsigned)Nq) return;
  const int ncap = max_pages << lps;
  const int L = min(max(kv_len[b], 0), ncap);
  const int p = L - Nq + (int)i;
  // the source: a uniform 64-bit base of the workgroup's first token, the lane's token and chunk on top
  const size_t tok = src_row_stride ? (size_t)src_row_stride : (size_t)D;
  const size_t base = (src_row_stride ? (size_t)b * (unsigned)Nq * tok + (size_t)h * D : (size_t)bh * (unsigned)Nq * tok) + (size_t)(tb * TPB) * tok;
  const size_t src = base + (size_t)r * tok + c * 8;
  const size_t srcp = base + (size_t)r * tok + rope_partner_chunk<INTERLEAVED>(c, rot_dim) * 8;   // the partner chunk of the same row
  const float* cs = cos_sin + (size_t)min(max(p, 0), max_pos - 1) * (unsigned)rot_dim;   // the row read is clamped: nothing outside the table
  if (isq) {
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(Qout + ((size_t)bh * (unsigned)Nq + i) * D + c * 8);
    if (p < 0) {                                                 // left padding: no visible key, a defined value
      *dst = u32x4_t{0u, 0u, 0u, 0u};
      return;
    }
    const u32x4_t q = *reinterpret_cast<const u32x4_t*>(Q + src);
    const u32x4_t qp = INTERLEAVED ? q : *reinterpret_cast<const u32x4_t*>(Q + srcp);
    *dst = rope_rotate8<INTERLEAVED>(q, qp, cs, c, rot_dim);
    return;
  }
  if (p < 0) return;                                             // left padding
  const int pid = block_table[(size_t)b * max_pages + (p >> lps)];   // p < L <= ncap: inside the table row
  if ((unsigned)pid >= (unsigned)num_pages) return;             // a bad page id drops the token
  const u32x4_t k = *reinterpret_cast<const u32x4_t*>(Knew + src);
  const u32x4_t kp = INTERLEAVED ? k : *reinterpret_cast<const u32x4_t*>(Knew + srcp);
  const u32x4_t v = *reinterpret_cast<const u32x4_t*>(Vnew + src);
  const u32x4_t kr = rope_rotate8<INTERLEAVED>(k, kp, cs, c, rot_dim);
  const size_t run = ((size_t)pid * (unsigned)Hkv + h) << lps;   // first row of the (page, head) run
  const unsigned off = (unsigned)(p & ((1 << lps) - 1)) * D + c * 8;   // elements inside the run
  if constexpr (KV8) {
    const float ks = k_scale ? k_scale[h] : 1.0f, vs = v_scale ? v_scale[h] : 1.0f;
    *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Kpool) + run * D + off) = kv8_quantize8(kr, ks);   // the codes of the row ROUNDED to fp16
    *reinterpret_cast<u32x2_t*>(static_cast<uint8_t*>(Vpool) + run * D + off) = kv8_quantize8(v, vs);
  } else {
    *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(Kpool) + run * D + off) = kr;
    *reinterpret_cast<u32x4_t*>(static_cast<half_t*>(Vpool) + run * D + off) = v;
  }
}

// grid: (B x Hkv + B x H) x bph workgroups of 256, bph = ceil(Nq / (2048 / D)), the first nkv = B x Hkv x bph of them K/V; lps = log2(page_size)
template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_paged_kernel(const half_t* Q, const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew,
                                                                half_t* Qout, half_t* __restrict__ Kpool, half_t* __restrict__ Vpool,
                                                                const float* __restrict__ cos_sin, const int* __restrict__ block_table,
                                                                const int* __restrict__ kv_len, int H, int Hkv, int Nq, int num_pages, int lps,
                                                                int max_pages, int bph, int rot_dim, int max_pos, long long src_row_stride,
                                                                unsigned nkv) {
  rope_append_paged_body<D, INTERLEAVED, false>(Q, Knew, Vnew, Qout, Kpool, Vpool, cos_sin, block_table, kv_len, nullptr, nullptr, H, Hkv, Nq, num_pages,
                                                lps, max_pages, bph, rot_dim, max_pos, src_row_stride, nkv);
}

template <int D, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_append_paged_kv8_kernel(const half_t* Q, const half_t* __restrict__ Knew, const half_t* __restrict__ Vnew,
                                                                    half_t* Qout, uint8_t* __restrict__ Kpool8, uint8_t* __restrict__ Vpool8,
                                                                    const float* __restrict__ cos_sin, const int* __restrict__ block_table,
                                                                    const int* __restrict__ kv_len, const float* __restrict__ k_scale,
                                                                    const float* __restrict__ v_scale, int H, int Hkv, int Nq, int num_pages, int lps,
                                                                    int max_pages, int bph, int rot_dim, int max_pos, long long src_row_stride,
                                                                    unsigned nkv) {
  rope_append_paged_body<D, INTERLEAVED, true>(Q, Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, block_table, kv_len, k_scale, v_scale, H, Hkv, Nq,
                                               num_pages, lps, max_pages, bph, rot_dim, max_pos, src_row_stride, nkv);
}

}  // namespace lc
