// attn_mla_sparse.hip — SPARSE multi-head latent attention: every query token attends to its own `topk` selected entries of the latent pools
// (DeepSeek-V3.2 "DSA", FlashMLA's `indices`; lc_attn_mla_sparse_f16 / _bf16).  slots[t, j] is the pool slot of key j of token
// t; an entry outside [0, num_slots) is not a key.  The arithmetic is attn_mla.hip's (§4.3q): fp32 products and softmax state, sm_scale log2 e
// on the fp32 scores, P rounded for the value product while the row sum keeps the unrounded value, O rounded once, lse in natural units.
//
//   - rows: only the H heads of ONE token share keys, so a workgroup (4 wave64) owns up to 64 heads of one token, 16 a wave (the dense split:
//     a 512 x 16 fp32 Oᵀ accumulator and 72 VGPRs of Q fragments a wave, nothing merged across waves); grid T x RB x S, RB = ceil(H / 64), S
//     ranges of the ceil(topk / 64) tiles.  Logical order (t, s, rb), rb fastest, under xcd_remap: the two row blocks of H = 128 and the
//     ranges of a token are neighbours in one XCD — they gather the same 1 KiB rows out of one L2
//   - the LDS image, its double buffer, the two staging halves, the Q fragments, the lane-local softmax and the one barrier per tile are
//     attn_mla.hip's.  Staging differs: wave w owns rows 16 w .. 16 w + 15 of the tile, latent AND rope part, so one wave answers for a row
//   - the entries of a tile: every wave reads the tile's 64 slots with ONE coalesced 256-byte load a tile ahead (lane j: entry 64 u + j; an
//     index behind topk reads the row's last entry and counts as -1).  A ballot of `0 <= slot < num_slots` is the tile's VALIDITY MASK in an
//     SGPR pair; it is the only thing that decides (a) the score mask (a select on bit 16 kb + 4 h + e), (b) what a staged row is and
//     (c) whether the wave loads at all.  A latent row is 1 KiB = one load instruction of the wave, so its slot is wave-uniform: v_readlane
//     puts it into an SGPR, the 64-bit base slot x 1024 lives in SGPRs; the two rope loads cover eight rows each, their slots come per lane
//     through ds_bpermute
//   - an INVALID entry contributes exactly nothing, whatever the pools hold: its load address is slot 0's (in bounds, never used) and the
//     value stored into the image is a select on the mask bit between the loaded registers and ZERO — pool data of an invalid entry never
//     reaches LDS, so neither MFMA sees it (0 x NaN cannot arise).  A wave whose 16 entries are all invalid issues no pool load at all: a
//     tile of -1 padding moves no pool data
//   - S == 1: O and lse written by the wave; S > 1: normalised fp32 partials and log2-domain lse into the workspace, merged by
//     attn_mla_sparse_combine_kernel over all T H rows (attn_mla_combine_kernel bounds its rows by cu_q, which this entry does not have)
#pragma once
#include "attn_mla.hip"   // MLA_* constants: the LDS image (attn_decode.hip: mfma16_16<BF16>, DEC_NEG_INF; lc_common.h: cvt16, lds_tr16, cat4, xcd_remap)

namespace lc {

template <bool BF16>
__global__ __launch_bounds__(256) void attn_mla_sparse_kernel(const half_t* __restrict__ Qc, const half_t* __restrict__ Qpe,
                                                              const half_t* __restrict__ CKV, const half_t* __restrict__ KPE,
                                                              half_t* __restrict__ O, float* __restrict__ lse, const int* __restrict__ slots,
                                                              float* __restrict__ part_o, float* __restrict__ part_lse, int H, int topk,
                                                              int num_slots, int S, float sl2, long total_rows) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;

  // ---- which (token, range, row block): logical id (t S + s) RB + rb, an XCD owning a contiguous eighth of the ids
  const int RB = __builtin_amdgcn_readfirstlane((H + 63) / 64);
  const int lid = __builtin_amdgcn_readfirstlane(xcd_remap((int)blockIdx.x, (int)gridDim.x));
  const int ts = __builtin_amdgcn_readfirstlane(lid / RB), rbase = 64 * (lid - ts * RB);   // (rbase < H: RB = ceil(H / 64))
  const int t = __builtin_amdgcn_readfirstlane(ts / S), s_idx = ts - t * S;
  const int Tw = (int)(((unsigned)topk + MLA_KT - 1) / MLA_KT);
  const int t0 = __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * Tw) / (unsigned)S));
  const int t1 = __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * Tw) / (unsigned)S));
  const int* __restrict__ srow = slots + (long)t * topk;

  // ---- this lane's head (heads >= H: head H - 1, nothing stored) and its 18 Q fragments: dims 32 s + 8 h ... of Qc, then of Qpe
  const bool wave_live = rbase + 16 * w < H;   // (wave-uniform)
  const int r = rbase + 16 * w + i16;
  const long grow = (long)t * H + (r < H ? r : H - 1);   // the row of Q, O and lse
  half8_t qf[MLA_KS];
#pragma unroll
  for (int s = 0; s < MLA_DC / 32; ++s) qf[s] = *reinterpret_cast<const half8_t*>(Qc + grow * MLA_DC + 32 * s + 8 * h);
#pragma unroll
  for (int s = 0; s < MLA_DR / 32; ++s) qf[MLA_DC / 32 + s] = *reinterpret_cast<const half8_t*>(Qpe + grow * MLA_DR + 32 * s + 8 * h);

  // ---- the entries of tile u, lane j: slots[t, 64 u + j]; an index behind topk is read inside the row and is -1 (64 u + 63 < topk + 63 < 2^32)
  auto fetch = [&](int u) {
    const unsigned j = (unsigned)u * MLA_KT + lane;
    const int v = srow[j < (unsigned)topk ? j : (unsigned)topk - 1];
    return j < (unsigned)topk ? v : -1;
  };
  auto valid_mask = [&](int sv) { return (unsigned long)__builtin_amdgcn_ballot_w64((unsigned)sv < (unsigned)num_slots); };
  auto wave_any = [&](unsigned long mask) { return ((mask >> (16 * w)) & 0xffffu) != 0; };   // (wave-uniform) one of this wave's 16 rows is a key

  // ---- tile staging.  CKV: load n of wave w is row 16 w + n of the tile, a lane its 16-byte chunk `lane` (1 KiB per instruction, the slot in
  // an SGPR); KPE: load n is rows 16 w + 8 n + (lane >> 3), chunk lane & 7, the slot per lane.  An invalid entry reads slot 0 and stores ZERO.
  // Two halves of nine loads a lane as in attn_mla.hip: A = CKV rows n = 0 .. 8, B = CKV rows n = 9 .. 15 and the two KPE loads
  u32x4_t stg[9];
#pragma unroll
  for (int n = 0; n < 9; ++n) stg[n] = u32x4_t{0u, 0u, 0u, 0u};
  auto ckv_src = [&](int sv, int n) {
    const int sl = __builtin_amdgcn_readlane(sv, 16 * w + n);
    const long row = (unsigned)sl < (unsigned)num_slots ? sl : 0;   // 64-bit: num_slots x 1024 may pass 2 GiB
    return reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(CKV) + row * (MLA_DC * 2) + lane * 16);
  };
  auto load_a = [&](int sv) {
#pragma unroll
    for (int n = 0; n < 9; ++n) stg[n] = *ckv_src(sv, n);
  };
  auto load_b = [&](int sv) {
#pragma unroll
    for (int n = 9; n < 16; ++n) stg[n - 9] = *ckv_src(sv, n);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int sl = __builtin_amdgcn_ds_bpermute(4 * (16 * w + 8 * n + (lane >> 3)), sv);
      const long row = (unsigned)sl < (unsigned)num_slots ? sl : 0;
      stg[7 + n] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(KPE) + row * (MLA_DR * 2) + (lane & 7) * 16);
    }
  };
  // what goes into the image is a select on the ENTRY's mask bit, never on pool data
  auto keep = [&](unsigned long mask, int row, u32x4_t v) { return ((mask >> row) & 1u) ? v : u32x4_t{0u, 0u, 0u, 0u}; };
  auto store_a = [&](char* img, unsigned long mask) {
#pragma unroll
    for (int n = 0; n < 9; ++n) *reinterpret_cast<u32x4_t*>(img + (16 * w + n) * MLA_ROW + lane * 16) = keep(mask, 16 * w + n, stg[n]);
  };
  auto store_b = [&](char* img, unsigned long mask) {
#pragma unroll
    for (int n = 9; n < 16; ++n) *reinterpret_cast<u32x4_t*>(img + (16 * w + n) * MLA_ROW + lane * 16) = keep(mask, 16 * w + n, stg[n - 9]);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int row = 16 * w + 8 * n + (lane >> 3);
      *reinterpret_cast<u32x4_t*>(img + row * MLA_ROW + MLA_DC * 2 + (lane & 7) * 16) = keep(mask, row, stg[7 + n]);
    }
  };

  float m = DEC_NEG_INF, l = 0.f;
  f32x4_t o[MLA_DB];
#pragma unroll
  for (int db = 0; db < MLA_DB; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // row read of the score product: key row i16 of a 16-key block, bytes 64 s + 16 h; transposed read of the value product: rows 4 h + q4 (+ 16)
  // of a 32-key step, 8 bytes at column 16 db + 4 p4
  const int k_off = i16 * MLA_ROW + 16 * h;
  const int tr_off = (4 * h + (i16 >> 2)) * MLA_ROW + 8 * (i16 & 3);

  unsigned long cur = 0;   // validity mask of the tile in the image being read
  int sv = -1;             // entries of the tile being staged
  if (t1 > t0) {
    sv = fetch(t0);
    cur = valid_mask(sv);
    if (wave_any(cur)) load_a(sv);
    store_a(lds, cur);
    if (wave_any(cur)) load_b(sv);
    store_b(lds, cur);
    sv = fetch(t0 + 1);
  }
  __syncthreads();
  // a wave without a head only moves data and meets the barriers (a loop of its own: attn_mla.hip)
  if (!wave_live) {
    for (int u = t0; u < t1; ++u) {
      char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
      if (u + 1 < t1) {
        const unsigned long nm = valid_mask(sv);
        if (wave_any(nm)) load_a(sv);
        store_a(nxt, nm);
        if (wave_any(nm)) load_b(sv);
        sv = fetch(u + 2);
        store_b(nxt, nm);
      }
      __syncthreads();
    }
    return;
  }
  for (int u = t0; u < t1; ++u) {
    char* img = lds + ((u - t0) & 1) * MLA_TILE;
    const bool more = u + 1 < t1;
    char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
    const unsigned long nm = more ? valid_mask(sv) : 0ul;
    const bool fill = wave_any(nm);
    // the first half of the next tile's loads, in flight under this tile's scores
    if (fill) load_a(sv);
    {
      // ---- Sᵀ = K Qᵀ: four 16-key blocks x 18 k-steps, the rope dims last
      f32x4_t st[4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < MLA_KS; ++s)
          acc = mfma16_16<BF16>(*reinterpret_cast<const half8_t*>(img + 16 * kb * MLA_ROW + k_off + 64 * s), qf[s], acc);
        st[kb] = acc;
      }
      // ---- online softmax in the log2 domain; register e of block kb is entry 64 u + 16 kb + 4 h + e: bit 16 kb + e of the lane's mask
      const unsigned long lm = cur >> (4 * h);
      float mx = DEC_NEG_INF;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = ((lm >> (16 * kb + e)) & 1u) ? st[kb][e] * sl2 : DEC_NEG_INF;   // select on the ENTRY: the score may be anything
          st[kb][e] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);
      const float mu = (mn == DEC_NEG_INF) ? 0.f : mn;   // no key yet: every exponent below is exp2(-inf) = 0
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
      // ---- the second half of the next tile's loads, in flight under the value product, and the entries of the tile behind it
      if (more) {
        store_a(nxt, nm);
        if (fill) load_b(sv);
        sv = fetch(u + 2);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- rescale Oᵀ only when some row's maximum moved (the empty statements: attn_mla.hip)
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int db = 0; db < MLA_DB; ++db) {
          asm volatile("" : "+a"(o[db]));
          o[db] *= alpha;
        }
      }
      // ---- Oᵀ += Vᵀ Pᵀ out of the SAME image: its first 1024 bytes a row, read transposed
#pragma unroll
      for (int db = 0; db < MLA_DB; ++db) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const half8_t va = cat4(lds_tr16(img + (32 * s) * MLA_ROW + tr_off + 32 * db), lds_tr16(img + (32 * s + 16) * MLA_ROW + tr_off + 32 * db));
          o[db] = mfma16_16<BF16>(va, pf[s], o[db]);
        }
      }
    }
    if (more) store_b(nxt, nm);
    cur = nm;
    __syncthreads();   // the next image is whole; every wave is done reading this one
  }

  // ---- a wave owns its heads: no merge across waves.  The four lane groups of a row hold disjoint keys: sum l once
  if (r >= H) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (S == 1) {
    half_t* dst = O + grow * MLA_DC + 4 * h;
#pragma unroll
    for (int db = 0; db < MLA_DB; ++db) {
      const f32x4_t x = o[db] * inv;
      const half4_t y = {cvt16<BF16>(x[0]), cvt16<BF16>(x[1]), cvt16<BF16>(x[2]), cvt16<BF16>(x[3])};
      *reinterpret_cast<half4_t*>(dst + 16 * db) = y;
    }
    if (lse && h == 0) lse[grow] = l > 0.f ? (m + log2f(l)) * 0.6931471805599453f : DEC_NEG_INF;
  } else {
    float* po = part_o + ((long)s_idx * total_rows + grow) * MLA_DC + 4 * h;
#pragma unroll
    for (int db = 0; db < MLA_DB; ++db) *reinterpret_cast<f32x4_t*>(po + 16 * db) = o[db] * inv;
    if (h == 0) part_lse[(long)s_idx * total_rows + grow] = l > 0.f ? m + log2f(l) : DEC_NEG_INF;
  }
}

// O[row] = sum_s w_s part_o[s][row] / sum_s w_s with w_s = exp2(lse_s - max lse) over ALL T H rows: weight 0 for a range without a key (its
// partial is never read), O = 0 and lse = -inf when no range has one; rounded once; lse (if asked) in natural units.
// One thread per (row, four columns): 128 threads a row, two rows a workgroup.
template <bool BF16>
__global__ __launch_bounds__(256) void attn_mla_sparse_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                      half_t* __restrict__ O, float* __restrict__ lse, long total_rows, int S) {
  constexpr int TPR = MLA_DC / 4;
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
      if (wgt > 0.f) {
        acc += *reinterpret_cast<const f32x4_t*>(part_o + ((long)s * total_rows + row) * MLA_DC + d) * wgt;
        ws += wgt;
      }
    }
  }
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  const half4_t y = {cvt16<BF16>(acc[0] * inv), cvt16<BF16>(acc[1] * inv), cvt16<BF16>(acc[2] * inv), cvt16<BF16>(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * MLA_DC + d) = y;
  if (lse && d == 0) lse[row] = mx == DEC_NEG_INF ? DEC_NEG_INF : (mx + log2f(ws)) * 0.6931471805599453f;
}

}  // namespace lc
