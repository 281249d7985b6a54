// attn_mla.hip — multi-head latent attention (MLA, the absorbed decode form of DeepSeek-V2 / V3 / R1, Kimi-K2) over a PAGED LATENT cache
// (lc_attn_mla_paged_f16 / _bf16).  The cache holds, per token, ONE 512-wide compressed latent row (CKV) and ONE 64-wide rotated
// key row (KPE), shared by every query head; scores are taken over 576 dims, values over 512, and the latent row is both key and value:
//   s_j = sm_scale (Qc . CKV_j + Qpe . KPE_j),   O = sum_j softmax_j(s) CKV_j,   lse = ln sum_j exp(s_j)
// on a ragged batch (cu_q, kv_len, block_table: the rules of attn_varlen.hip, §4.3l).  No device code is shared with the decode body.
//
//   - rows: r = h Nq_b + i of the [H Nq_b] row matrix of a sequence (the varlen order); a workgroup (4 wave64) owns a block of up to 64 of them
//     and its four waves split the ROWS, 16 each; EVERY wave walks ALL keys of the workgroup's range.  So a wave's Oᵀ accumulator is 512 x 16
//     fp32 = 128 registers a lane (the decode body's split — waves over keys, a full [rows x D] accumulator per wave — would need 512), its
//     Q fragments (16 rows x 576: 18 k-steps of 8 halves) stay in 72 VGPRs for the whole walk, and nothing is merged across waves at the end
//   - the latent tile is read ONCE: a 64-key tile [64 x (512 + 64)] goes from HBM into ONE LDS image (rows of 1152 + 16 bytes: the padding
//     spreads the 16 rows of a fragment read over the banks), double-buffered.  That image is the A operand of Sᵀ = K Qᵀ (ds_read_b128 row
//     reads; the 64 rope dims are the last two 32-wide k-steps of the same accumulation) AND the A operand of Oᵀ += Vᵀ Pᵀ (ds_read_b64_tr_b16
//     transposed reads of its first 1024 bytes a row).  No second copy, no second load
//   - Sᵀ = K Qᵀ leaves a lane ONE query row (lane & 15) and 16 keys of the tile: P is, register for register, the B operand of Oᵀ += Vᵀ Pᵀ
//     (the lane-local softmax of §4.3); sm_scale log2 e is applied to the fp32 SCORES (one multiply a score), not folded into Q: a bf16 Q is
//     not rounded a second time
//   - tiles are staged through registers in two halves of nine 16-byte loads a lane (36 VGPRs in flight: next to 128 accumulators and 72 of Q a
//     whole tile's 72 made hipcc park loaded values in AGPRs and wait for them early): half A of tile u + 1 is issued in front of the scores
//     of tile u and stored into the other image behind them, half B is in flight under the value product; ONE barrier per tile.  A wave
//     loads whole key rows (1 KiB per load instruction), so a row's page is wave-uniform: table entries are scalar loads one tile ahead, page
//     bases live in SGPRs.  A tile may span pages (page_size >= 16: a 16-key block never does)
//   - source rows are clamped to the last walked key and never zero-filled; a masked score is a SELECT on the key index (P = 0 exactly); page
//     ids are clamped into the pool in the kernel; table entries behind ceil(L_b / page_size) are not read
//   - grid: B x RB x S workgroups, RB = ceil(H max_nq / 64) row blocks, S key ranges (tiles [s Tw / S, (s + 1) Tw / S) of the Tw tiles the
//     block walks: causal, only the keys its last row sees).  The LOGICAL order is (b, s, rb), rb fastest, and hardware block ids are mapped
//     onto it by xcd_remap: an XCD owns a contiguous eighth, so the row blocks of one (sequence, range) — which read the same K / V — meet in
//     one L2, and the live blocks of a mostly empty ragged grid spread over all XCDs (§4.3l, finding 3)
//   - a workgroup whose block starts at or past H Nq_b returns in front of its first LDS access and barrier; a wave without a row keeps
//     loading and meeting barriers and skips the arithmetic
//   - S == 1: the wave normalises, rounds ONCE (RNE) and writes O and, if asked, lse (natural units).  S > 1: the NORMALISED fp32 partial and
//     the row's log2-domain log-sum-exp (-inf: no visible key in the range) go to the workspace, attn_mla_combine_kernel merges them
#pragma once
#include "attn_decode.hip"   // mfma16_16<BF16>, DEC_NEG_INF (lc_common.h: cvt16<BF16>, lds_tr16, cat4, xcd_remap)

namespace lc {

constexpr int MLA_DC = 512;                            // latent (value) dims
constexpr int MLA_DR = 64;                             // rope dims
constexpr int MLA_KT = 64;                             // keys per tile
constexpr int MLA_ROW = (MLA_DC + MLA_DR) * 2 + 16;    // bytes of a key row in the LDS image: 1152 + 16 of padding
constexpr int MLA_TILE = MLA_KT * MLA_ROW;             // 74 752 bytes; two images: 149 504 of the 163 840
constexpr int MLA_KS = (MLA_DC + MLA_DR) / 32;         // 18 k-steps of a score
constexpr int MLA_DB = MLA_DC / 16;                    // 32 blocks of 16 output columns
constexpr int MLA_LDS = 2 * MLA_TILE;

template <bool BF16>
__global__ __launch_bounds__(256) void attn_mla_paged_kernel(const half_t* __restrict__ Qc, const half_t* __restrict__ Qpe,
                                                             const half_t* __restrict__ CKV, const half_t* __restrict__ KPE,
                                                             half_t* __restrict__ O, float* __restrict__ lse, const int* __restrict__ cu_q,
                                                             const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                             float* __restrict__ part_o, float* __restrict__ part_lse, int H, int T, int max_nq,
                                                             int num_pages, int lps, int max_pages, int causal, int S, float sl2,
                                                             long total_rows) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;

  // ---- which (sequence, key range, row block): logical id (b S + s) RB + rb, an XCD owning a contiguous eighth of the ids
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
  // the keys this block walks: all L_b, or (causal) those its last token sees — i_max is Nq_b - 1 where the block straddles a head boundary
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

  // ---- this lane's query row (rows >= R: row R - 1, nothing stored) and its 18 Q fragments: dims 32 s + 8 h ... of Qc, then of Qpe
  const bool wave_live = rbase + 16 * w < R;   // (wave-uniform)
  const int r = rbase + 16 * w + i16;
  const int rs = r < R ? r : R - 1;
  const int hq = rs / Nqb, iq = rs - hq * Nqb;
  const long grow = (long)(q0 + iq) * H + hq;   // the row of Q, O and lse (q0 + iq < T: the clamps above)
  half8_t qf[MLA_KS];
#pragma unroll
  for (int s = 0; s < MLA_DC / 32; ++s) qf[s] = *reinterpret_cast<const half8_t*>(Qc + grow * MLA_DC + 32 * s + 8 * h);
#pragma unroll
  for (int s = 0; s < MLA_DR / 32; ++s) qf[MLA_DC / 32 + s] = *reinterpret_cast<const half8_t*>(Qpe + grow * MLA_DR + 32 * s + 8 * h);
  int lim = causal ? Lb - Nqb + iq + 1 : Lb;   // keys j < lim are visible to this row
  lim = lim < 0 ? 0 : lim;

  // ---- tile staging.  CKV: load n of wave w is key row 4 n + w of the tile, a lane its 16-byte chunk `lane` (1 KiB per instruction);
  // KPE: load n is rows 32 n + 8 w + (lane >> 3), chunk lane & 7.  The page of a 16-key block is wave-uniform
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
  // two halves of nine loads a lane: A = CKV rows n = 0 .. 8, B = CKV rows n = 9 .. 15 and the two KPE loads (36 VGPRs in flight at a time:
  // with 128 accumulators and 72 of Q a whole tile's 72 does not fit — hipcc then parks loaded values in AGPRs and waits for them early)
  u32x4_t stg[9];
  auto ckv_src = [&](int u, int n) {
    int key = u * MLA_KT + 4 * n + w;
    key = key < last ? key : last;
    const char* base = reinterpret_cast<const char*>(CKV) + (((long)pid[n >> 2] << lps) * (MLA_DC * 2));
    return reinterpret_cast<const u32x4_t*>(base + ((unsigned)(key & pmask) * (MLA_DC * 2) + lane * 16));
  };
  auto load_a = [&](int u) {
#pragma unroll
    for (int n = 0; n < 9; ++n) stg[n] = *ckv_src(u, n);
  };
  auto load_b = [&](int u) {
#pragma unroll
    for (int n = 9; n < 16; ++n) stg[n - 9] = *ckv_src(u, n);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      int key = u * MLA_KT + 32 * n + 8 * w + (lane >> 3);
      key = key < last ? key : last;
      const int id = (w >> 1) ? pid[2 * n + 1] : pid[2 * n];
      const char* base = reinterpret_cast<const char*>(KPE) + (((long)id << lps) * (MLA_DR * 2));
      stg[7 + n] = *reinterpret_cast<const u32x4_t*>(base + ((unsigned)(key & pmask) * (MLA_DR * 2) + (lane & 7) * 16));
    }
  };
  auto store_a = [&](char* img) {
#pragma unroll
    for (int n = 0; n < 9; ++n) *reinterpret_cast<u32x4_t*>(img + (4 * n + w) * MLA_ROW + lane * 16) = stg[n];
  };
  auto store_b = [&](char* img) {
#pragma unroll
    for (int n = 9; n < 16; ++n) *reinterpret_cast<u32x4_t*>(img + (4 * n + w) * MLA_ROW + lane * 16) = stg[n - 9];
#pragma unroll
    for (int n = 0; n < 2; ++n)
      *reinterpret_cast<u32x4_t*>(img + (32 * n + 8 * w + (lane >> 3)) * MLA_ROW + MLA_DC * 2 + (lane & 7) * 16) = stg[7 + n];
  };

  float m = DEC_NEG_INF, l = 0.f;
  f32x4_t o[MLA_DB];
#pragma unroll
  for (int db = 0; db < MLA_DB; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // row read of the score product: key row i16 of a 16-key block, bytes 64 s + 16 h; transposed read of the value product: rows 4 h + q4 (+ 16)
  // of a 32-key step, 8 bytes at column 16 db + 4 p4
  const int k_off = i16 * MLA_ROW + 16 * h;
  const int tr_off = (4 * h + (i16 >> 2)) * MLA_ROW + 8 * (i16 & 3);

  if (t1 > t0) {
    page_ids(t0);
    load_a(t0);
    store_a(lds);
    load_b(t0);
    store_b(lds);
    page_ids(t0 + 1);
  }
  __syncthreads();
  // a wave without a row only moves data and meets the barriers.  A loop of its own: with a branch on wave_live inside the arithmetic loop
  // hipcc carried the 128 accumulators through the VALU on every tile
  if (!wave_live) {
    for (int u = t0; u < t1; ++u) {
      char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
      if (u + 1 < t1) {
        load_a(u + 1);
        store_a(nxt);
        load_b(u + 1);
        page_ids(u + 2);
        store_b(nxt);
      }
      __syncthreads();
    }
    return;
  }
  for (int u = t0; u < t1; ++u) {
    char* img = lds + ((u - t0) & 1) * MLA_TILE;
    const bool more = u + 1 < t1;
    char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
    // the first half of the next tile's loads, in flight under this tile's scores
    if (more) load_a(u + 1);
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
      // ---- the second half of the next tile's loads, in flight under the value product, and the table entries of the tile behind it
      if (more) {
        store_a(nxt);
        load_b(u + 1);
        page_ids(u + 2);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- rescale Oᵀ only when some row's maximum moved (a multiplication by exactly 1 otherwise: same bits)
      // (the empty statements name the accumulators where the MFMAs keep them: without them hipcc hoists the 128 AGPR reads of this block
      // to the head of the loop, where they run on every tile and hold 128 VGPRs through the scores)
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
    if (more) store_b(nxt);
    __syncthreads();   // the next image is whole; every wave is done reading this one
  }

  // ---- a wave owns its rows: no merge across waves.  The four lane groups of a row hold disjoint keys: sum l once
  if (r >= R) return;
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

// O[row] = sum_s w_s part_o[s][row] / sum_s w_s with w_s = exp2(lse_s - max lse): weight 0 for a range without a visible key (its partial is
// never read), O = 0 and lse = -inf when no range has one; rounded once; lse (if asked) in natural units.  Only the rows of the tokens
// clamp(cu_q[0], 0, T) ... clamp(cu_q[B], 0, T) - 1: the range kernels wrote no partial for a token outside them, and its O row is nobody's.
// One thread per (row, four columns): 128 threads a row, two rows a workgroup.
template <bool BF16>
__global__ __launch_bounds__(256) void attn_mla_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                               half_t* __restrict__ O, float* __restrict__ lse, const int* __restrict__ cu_q,
                                                               int B, int T, int H, int S) {
  constexpr int TPR = MLA_DC / 4;
  const long row = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  const int d = (threadIdx.x % TPR) * 4;
  const int beg = cu_q[0], end = cu_q[B];
  const long total_rows = (long)T * H;
  if (row < (long)(beg < 0 ? 0 : (beg > T ? T : beg)) * H) return;
  if (row >= (long)(end < 0 ? 0 : (end > T ? T : end)) * H) return;
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
