// attn_mla_kv8.hip — multi-head latent attention over a paged latent cache whose LATENT rows are fp8 (lc_attn_mla_paged_kv8 / _kv8_bf16;
// DESIGN.md §4.3r).  CKV is [num_pages, page_size, 512] OCP e4m3fn bytes, an element's value is code x ckv_scale[0]; KPE stays 16-bit in the
// element type of Q.  What is computed, the ragged batch, the clamps, the grid, the row split over four waves, the 128 Oᵀ accumulators, the 72
// registers of Q, the lane-local softmax and the ONE LDS image read by rows for the scores and transposed for the values are attn_mla.hip's
// (§4.3q); its constants and attn_mla_combine_kernel<BF16> are used from there.  What is this kernel's own:
//   - a WHOLE 64-key tile is staged per round trip: a latent row is 512 bytes, so a tile is ten 16-byte loads a lane (eight of codes, two of
//     rope halves; 40 VGPRs where the 16-bit kernel holds half a tile in 36).  All ten of tile u + 1 are issued at the top of tile u, in
//     front of the scores, and converted and stored into the other image behind the value product, in front of the tile's one barrier
//   - latent load n of wave w is key rows 8 n + 2 w + (lane >> 5) of the tile, chunk lane & 31 (16 codes): two contiguous 512-byte rows per
//     instruction, both inside one 16-key block, so the page is wave-uniform and the page bases stay in SGPRs.  The rope loads keep their map
//   - codes are converted ONCE, at staging: 16 codes -> two kv8_16x8<BF16> results (exact for both element types) -> two 16-byte LDS writes
//     at row MLA_ROW + 32 chunk.  The image is byte for byte the one attn_mla_paged_kernel builds from a pool of the unscaled code values
//   - the scale is applied in fp32, where a power of two changes no bit: a score chain runs its 16 latent k-steps, is multiplied by the
//     scale and CONTINUES with the two rope k-steps; the values accumulate unscaled codes and are multiplied by the scale once in the
//     epilogue, behind the multiply by 1 / l (the rounded output and the fp32 partial alike).  ckv_scale is read once per workgroup by the
//     kernel (NULL: 1.0), so a replayed graph sees a new scale; a NaN, zero or negative scale is the caller's business
// The score / softmax / value block is stated a second time here rather than shared with attn_mla.hip: the staging calls and the scale sit
// inside it, and attn_mla_paged_kernel's assembly stays what it was.
#pragma once
#include "attn_mla.hip"   // MLA_* constants, attn_mla_combine_kernel<BF16> (attn_decode.hip: kv8_16x8<BF16>, mfma16_16<BF16>)

namespace lc {

template <bool BF16>
__global__ __launch_bounds__(256) void attn_mla_paged_kv8_kernel(const half_t* __restrict__ Qc, const half_t* __restrict__ Qpe,
                                                                 const uint8_t* __restrict__ CKV, const half_t* __restrict__ KPE,
                                                                 half_t* __restrict__ O, float* __restrict__ lse, const int* __restrict__ cu_q,
                                                                 const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                                 const float* __restrict__ ckv_scale, float* __restrict__ part_o,
                                                                 float* __restrict__ part_lse, int H, int T, int max_nq, int num_pages, int lps,
                                                                 int max_pages, int causal, int S, float sl2, long total_rows) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;

  // ---- which (sequence, key range, row block): attn_mla_paged_kernel's logical order
  const int RB = __builtin_amdgcn_readfirstlane((H * max_nq + 63) / 64);
  const int lid = __builtin_amdgcn_readfirstlane(xcd_remap((int)blockIdx.x, (int)gridDim.x));
  const int bs = __builtin_amdgcn_readfirstlane(lid / RB), rbase = 64 * (lid - bs * RB);
  const int b = __builtin_amdgcn_readfirstlane(bs / S), s_idx = bs - b * S;
  const int c0 = __builtin_amdgcn_readfirstlane(cu_q[b]), c1 = __builtin_amdgcn_readfirstlane(cu_q[b + 1]);
  const int q0 = c0 < 0 ? 0 : (c0 > T ? T : c0);
  const int cap = max_nq < T - q0 ? max_nq : T - q0;
  const int Nqb = c1 <= q0 ? 0 : (c1 - q0 > cap ? cap : c1 - q0);
  const int R = H * Nqb;
  if (rbase >= R) return;   // no row of this sequence in the block (Nq_b = 0 included): nothing touched, no barrier met
  const int Ncap = max_pages << lps;
  int Lb = __builtin_amdgcn_readfirstlane(kv_len[b]);
  Lb = Lb < 0 ? 0 : (Lb > Ncap ? Ncap : Lb);
  int Lw = Lb;
  if (causal) {
    const int span = (R - rbase < 64 ? R - rbase : 64) - 1;
    const int i0 = __builtin_amdgcn_readfirstlane(rbase % Nqb);
    const int imax = i0 + span >= Nqb ? Nqb - 1 : i0 + span;
    const int v = Lb - Nqb + imax + 1;
    Lw = v < 0 ? 0 : (v > Lb ? Lb : v);
  }
  const int Tw = (Lw + MLA_KT - 1) / MLA_KT;
  const int t0 = __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * Tw) / (unsigned)S));
  const int t1 = __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * Tw) / (unsigned)S));
  const int last = Lw - 1;   // (>= 0 whenever a tile exists)
  // the latent scale: one scalar load per workgroup
  const float sc = ckv_scale ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ckv_scale[0]))) : 1.f;

  // ---- this lane's query row (rows >= R: row R - 1, nothing stored) and its 18 Q fragments
  const bool wave_live = rbase + 16 * w < R;   // (wave-uniform)
  const int r = rbase + 16 * w + i16;
  const int rs = r < R ? r : R - 1;
  const int hq = rs / Nqb, iq = rs - hq * Nqb;
  const long grow = (long)(q0 + iq) * H + hq;
  half8_t qf[MLA_KS];
#pragma unroll
  for (int s = 0; s < MLA_DC / 32; ++s) qf[s] = *reinterpret_cast<const half8_t*>(Qc + grow * MLA_DC + 32 * s + 8 * h);
#pragma unroll
  for (int s = 0; s < MLA_DR / 32; ++s) qf[MLA_DC / 32 + s] = *reinterpret_cast<const half8_t*>(Qpe + grow * MLA_DR + 32 * s + 8 * h);
  int lim = causal ? Lb - Nqb + iq + 1 : Lb;   // keys j < lim are visible to this row
  lim = lim < 0 ? 0 : lim;

  // ---- tile staging: ten loads a lane, a whole tile.  CKV: load n of wave w is key rows 8 n + 2 w + (lane >> 5), chunk lane & 31 (1 KiB per
  // instruction, inside the 16-key block n >> 1); KPE: load n is rows 32 n + 8 w + (lane >> 3), chunk lane & 7
  const int pmask = (1 << lps) - 1;
  int pid[4];
  auto page_ids = [&](int u) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      int first = u * MLA_KT + 16 * kb;
      first = first < last ? first : last;   // (a block past the last key names the last key's page: always a table position below ceil(L_b / page_size))
      int id = __builtin_amdgcn_readfirstlane(block_table[(long)b * max_pages + (first >> lps)]);
      id = id < 0 ? 0 : id;
      pid[kb] = id < num_pages ? id : num_pages - 1;
    }
  };
  u32x4_t stg[10];
  const int crow = 2 * w + (lane >> 5), cchunk = lane & 31;
  auto load_tile = [&](int u) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      int key = u * MLA_KT + 8 * n + crow;
      key = key < last ? key : last;
      const char* base = reinterpret_cast<const char*>(CKV) + (((long)pid[n >> 1] << lps) * MLA_DC);
      stg[n] = *reinterpret_cast<const u32x4_t*>(base + ((unsigned)(key & pmask) * MLA_DC + cchunk * 16));
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      int key = u * MLA_KT + 32 * n + 8 * w + (lane >> 3);
      key = key < last ? key : last;
      const int id = (w >> 1) ? pid[2 * n + 1] : pid[2 * n];
      const char* base = reinterpret_cast<const char*>(KPE) + (((long)id << lps) * (MLA_DR * 2));
      stg[8 + n] = *reinterpret_cast<const u32x4_t*>(base + ((unsigned)(key & pmask) * (MLA_DR * 2) + (lane & 7) * 16));
    }
  };
  auto store_tile = [&](char* img) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      char* dst = img + (8 * n + crow) * MLA_ROW + 32 * cchunk;
      *reinterpret_cast<u32x4_t*>(dst) = kv8_16x8<BF16>(stg[n][0], stg[n][1]);
      *reinterpret_cast<u32x4_t*>(dst + 16) = kv8_16x8<BF16>(stg[n][2], stg[n][3]);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
      *reinterpret_cast<u32x4_t*>(img + (32 * n + 8 * w + (lane >> 3)) * MLA_ROW + MLA_DC * 2 + (lane & 7) * 16) = stg[8 + n];
  };

  float m = DEC_NEG_INF, l = 0.f;
  f32x4_t o[MLA_DB];
#pragma unroll
  for (int db = 0; db < MLA_DB; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int k_off = i16 * MLA_ROW + 16 * h;
  const int tr_off = (4 * h + (i16 >> 2)) * MLA_ROW + 8 * (i16 & 3);

  if (t1 > t0) {
    page_ids(t0);
    load_tile(t0);
    // Q is in its registers from here on (the empty statements use it, in front of the first tile's stores so that both sets of loads share
    // one round trip): hipcc otherwise sinks the 18 loads behind the branch below, and the loop's counted waits for them — vmcnt(17) ...
    // vmcnt(0) in its score chain — would then drain the staged tile on every iteration
#pragma unroll
    for (int s = 0; s < MLA_KS; ++s) asm volatile("" ::"v"(qf[s]));
    store_tile(lds);
    page_ids(t0 + 1);
  }
#pragma unroll
  for (int s = 0; s < MLA_KS; ++s) asm volatile("" ::"v"(qf[s]));   // (... on the path without a tile too: the waits are decided per path)
  __syncthreads();
  // a wave without a row only moves data and meets the barriers (a loop of its own: §4.3q)
  if (!wave_live) {
    for (int u = t0; u < t1; ++u) {
      char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
      if (u + 1 < t1) {
        load_tile(u + 1);
        page_ids(u + 2);
        store_tile(nxt);
      }
      __syncthreads();
    }
    return;
  }
  for (int u = t0; u < t1; ++u) {
    char* img = lds + ((u - t0) & 1) * MLA_TILE;
    const bool more = u + 1 < t1;
    char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
    // the whole next tile's loads, in flight under this tile's scores and value product
    if (more) load_tile(u + 1);
    {
      // ---- Sᵀ = K Qᵀ: four 16-key blocks; 16 latent k-steps on the codes, the scale, then the two rope k-steps of the SAME chain
      f32x4_t st[4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < MLA_DC / 32; ++s)
          acc = mfma16_16<BF16>(*reinterpret_cast<const half8_t*>(img + 16 * kb * MLA_ROW + k_off + 64 * s), qf[s], acc);
        acc *= sc;
#pragma unroll
        for (int s = MLA_DC / 32; s < MLA_KS; ++s)
          acc = mfma16_16<BF16>(*reinterpret_cast<const half8_t*>(img + 16 * kb * MLA_ROW + k_off + 64 * s), qf[s], acc);
        st[kb] = acc;
      }
      // ---- online softmax in the log2 domain; register e of block kb is key 64 u + 16 kb + 4 h + e
      const int k0 = u * MLA_KT + 4 * h;
      float mx = DEC_NEG_INF;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = k0 + 16 * kb + e < lim ? st[kb][e] * sl2 : DEC_NEG_INF;   // select on the INDEX: the score may be anything
          st[kb][e] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);
      const float mu = (mn == DEC_NEG_INF) ? 0.f : mn;   // no visible key yet: every exponent below is exp2(-inf) = 0
      const float alpha = __builtin_amdgcn_exp2f(m - mu);
      m = mn;
      float ps = 0.f;
      half8_t pf[2];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = __builtin_amdgcn_exp2f(st[kb][e] - mu);
          ps += p;   // (the row sum keeps the unrounded value)
          pf[kb >> 1][4 * (kb & 1) + e] = cvt16<BF16>(p);
        }
      l = l * alpha + ps;
      __builtin_amdgcn_sched_barrier(0);
      // ---- the table entries of the tile behind the one in flight
      if (more) page_ids(u + 2);
      __builtin_amdgcn_sched_barrier(0);
      // ---- rescale Oᵀ only when some row's maximum moved (the empty statements: §4.3q)
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int db = 0; db < MLA_DB; ++db) {
          asm volatile("" : "+a"(o[db]));
          o[db] *= alpha;
        }
      }
      // ---- Oᵀ += Vᵀ Pᵀ out of the SAME image (unscaled code values): its first 1024 bytes a row, read transposed
#pragma unroll
      for (int db = 0; db < MLA_DB; ++db) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const half8_t va = cat4(lds_tr16(img + (32 * s) * MLA_ROW + tr_off + 32 * db), lds_tr16(img + (32 * s + 16) * MLA_ROW + tr_off + 32 * db));
          o[db] = mfma16_16<BF16>(va, pf[s], o[db]);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- convert the next tile once and store it: 64 conversions and 18 LDS writes a lane
    if (more) store_tile(nxt);
    __syncthreads();   // the next image is whole; every wave is done reading this one
  }

  // ---- a wave owns its rows: no merge across waves.  The scale comes behind the multiply by 1 / l
  if (r >= R) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (S == 1) {
    half_t* dst = O + grow * MLA_DC + 4 * h;
#pragma unroll
    for (int db = 0; db < MLA_DB; ++db) {
      const f32x4_t x = (o[db] * inv) * sc;
      const half4_t y = {cvt16<BF16>(x[0]), cvt16<BF16>(x[1]), cvt16<BF16>(x[2]), cvt16<BF16>(x[3])};
      *reinterpret_cast<half4_t*>(dst + 16 * db) = y;
    }
    if (lse && h == 0) lse[grow] = l > 0.f ? (m + log2f(l)) * 0.6931471805599453f : DEC_NEG_INF;
  } else {
    float* po = part_o + ((long)s_idx * total_rows + grow) * MLA_DC + 4 * h;
#pragma unroll
    for (int db = 0; db < MLA_DB; ++db) *reinterpret_cast<f32x4_t*>(po + 16 * db) = (o[db] * inv) * sc;
    if (h == 0) part_lse[(long)s_idx * total_rows + grow] = l > 0.f ? m + log2f(l) : DEC_NEG_INF;
  }
}

}  // namespace lc
