// mla_index_logits.hip — the index logits of DeepSeek-V3.2's "lightning indexer" over a PAGED index-key pool (lc_mla_index_logits_f16 / _bf16;
// DESIGN.md §4.3u): for query token t of sequence b and visible key position j
//   logit[t, j] = sum_{h < 64} w[t, h] max(0, sum_{d < 128} Qi[t, h, d] Ki[slot(b, j), d])
// on a ragged batch (cu_q, kv_len, block_table: the rules of attn_mla.hip, §4.3q).  fp32 throughout: MFMA accumulation, relu, ONE multiply by
// w, the sum over heads; nothing is rounded to 16 bits.  There is no softmax state, no dependency between tiles and no reduction over keys:
// key ranges are grid entries, no combine kernel, no workspace.
//
//   - rows: the 64 index heads of a token are the only rows that share a product; all tokens of a sequence share the keys.  A workgroup (4
//     wave64) owns a block of up to IDX_TB = 8 consecutive query tokens of ONE sequence and a range of 64-key tiles; a key tile goes from
//     HBM / L2 into LDS once per token block, not once per token
//   - ONE scheme for prefill and decode: the block's tokens form np = ceil(nt / 2) PAIRS; with npp = 1, 2 or 4 (np rounded up to a power of
//     two) wave w owns pair w % npp and the 16-key blocks kb = w / npp, w / npp + 4 / npp, ... of every tile.  Eight tokens: a wave a pair,
//     all four key blocks.  One token (a decode step): all four waves hold the token and split the tile's four 16-key blocks — every wave has
//     arithmetic.  A second scheme would differ in nothing but these three wave-uniform numbers
//   - the swapped product: Qi is the ROW operand of v_mfma_f32_16x16x32, the key block the column operand, so a lane holds ONE key (lane & 15)
//     and the four heads 16 hb + 4 (lane >> 4) + e of each of the four head blocks hb: relu, the multiply by w and the sum over its 16 heads
//     are lane-local, the sum over the four lane groups is two cross-lane steps.  A token's Qi: 16 fragments = 64 VGPRs, read once; its w: 16
//     floats a lane, read once.  A 16-key block's fragments (16 VGPRs) are read from LDS once and serve both tokens of the pair
//   - data movement: a key row is 256 bytes, a tile 16 KiB (LDS rows of 256 + 16 bytes: the padding spreads a fragment read's 16 rows over the
//     banks), double-buffered: 34 816 bytes.  Four 16-byte loads a lane a tile, issued in front of the tile's arithmetic and stored behind
//     it; ONE barrier per tile.  Load n of wave w is rows 16 n + 4 w + (lane >> 4) of the tile, chunk lane & 15: a 16-key block never
//     straddles a page (page_size >= 16), so its page id is a scalar load one tile ahead and its 64-bit base lives in SGPRs
//   - source rows are clamped to the last walked key; page ids are clamped into the pool; table entries behind ceil(L_b / page_size) are
//     not read.  The causal edge masks the STORE, never the product: the tokens of a block see different n_t, the block walks the keys its
//     last token sees
//   - grid: B x NB x S workgroups, NB = ceil(max_nq / 8) token blocks, S key ranges (tiles [s Tw / S, (s + 1) Tw / S) of the Tw tiles the
//     block walks).  Logical order (b, s, nb), nb fastest, under xcd_remap: the token blocks that read the same key range meet in one L2
//   - a workgroup whose block starts at or past Nq_b returns in front of its first LDS access and barrier
#pragma once
#include "attn_decode.hip"   // mfma16_16<BF16> (lc_common.h: xcd_remap, wave_id)

namespace lc {

constexpr int IDX_H = 64;                       // index heads
constexpr int IDX_D = 128;                      // index head dim
constexpr int IDX_KT = 64;                      // keys per tile
constexpr int IDX_TB = 8;                       // query tokens per workgroup: a pair a wave
constexpr int IDX_ROW = IDX_D * 2 + 16;         // bytes of a key row in the LDS image: 256 + 16 of padding
constexpr int IDX_TILE = IDX_KT * IDX_ROW;      // 17 408 bytes
constexpr int IDX_LDS = 2 * IDX_TILE;           // 34 816 of the 163 840
constexpr int IDX_KS = IDX_D / 32;              // 4 k-steps
constexpr int IDX_HB = IDX_H / 16;              // 4 head blocks

template <bool BF16>
__global__ __launch_bounds__(256) void mla_index_logits_kernel(const half_t* __restrict__ Qi, const float* __restrict__ wgt,
                                                               const half_t* __restrict__ Ki, float* __restrict__ logits,
                                                               const int* __restrict__ cu_q, const int* __restrict__ block_table,
                                                               const int* __restrict__ kv_len, int T, int max_nq, int num_pages, int lps,
                                                               int max_pages, int causal, int S, int NB, long ld) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;

  // ---- which (sequence, key range, token block): logical id (b S + s) NB + nb, an XCD owning a contiguous eighth of the ids
  const int lid = __builtin_amdgcn_readfirstlane(xcd_remap((int)blockIdx.x, (int)gridDim.x));
  const int bs = __builtin_amdgcn_readfirstlane(lid / NB), nb = lid - bs * NB;
  const int b = __builtin_amdgcn_readfirstlane(bs / S), s_idx = bs - b * S;
  const int c0 = __builtin_amdgcn_readfirstlane(cu_q[b]), c1 = __builtin_amdgcn_readfirstlane(cu_q[b + 1]);
  const int q0 = c0 < 0 ? 0 : (c0 > T ? T : c0);
  const int cap = max_nq < T - q0 ? max_nq : T - q0;
  const int Nqb = c1 <= q0 ? 0 : (c1 - q0 > cap ? cap : c1 - q0);
  const int ib = nb * IDX_TB;   // the block's first token of the sequence
  if (ib >= Nqb) return;        // no token of this sequence in the block (Nq_b = 0 included): nothing touched, no barrier met
  const int Ncap = max_pages << lps;
  int Lb = __builtin_amdgcn_readfirstlane(kv_len[b]);
  Lb = Lb < 0 ? 0 : (Lb > Ncap ? Ncap : Lb);
  const int nt = Nqb - ib < IDX_TB ? Nqb - ib : IDX_TB;   // tokens of the block: 1 .. 8
  // keys j < n(i) are visible to token i of the sequence; the block walks those of its last token
  auto visible = [&](int i) {
    const int v = causal ? Lb - Nqb + i + 1 : Lb;
    return v < 0 ? 0 : (v > Lb ? Lb : v);
  };
  const int Lw = visible(ib + nt - 1);
  const int Tw = (Lw + IDX_KT - 1) / IDX_KT;
  const int t0 = __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * Tw) / (unsigned)S));
  const int t1 = __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * Tw) / (unsigned)S));
  const int last = Lw - 1;   // (>= 0 whenever a tile exists)

  // ---- the wave's pair of tokens and its 16-key blocks of a tile (all wave-uniform)
  const int np = (nt + 1) >> 1;
  const int npp = np == 1 ? 1 : (np == 2 ? 2 : 4);
  const int pair = w & (npp - 1), kb0 = w / npp, kstep = 4 / npp;
  const bool wave_live = pair < np;                                   // (np = 3: the fourth wave only moves data)
  const int ia = ib + 2 * (wave_live ? pair : 0);                     // the pair's first token; its second one exists when ia + 1 < ib + nt
  const bool two = wave_live && ia + 1 < ib + nt;
  const int tok[2] = {q0 + ia, q0 + (two ? ia + 1 : ia)};             // (< T: the clamps above)
  const int nvis[2] = {wave_live ? visible(ia) : 0, two ? visible(ia + 1) : 0};

  // ---- Q fragments of the pair: head 16 hb + i16, dims 32 s + 8 h ...; w: heads 16 hb + 4 h + e
  half8_t qf[2][IDX_HB * IDX_KS];
  f32x4_t wf[2][IDX_HB];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const half_t* qrow = Qi + ((long)tok[k] * IDX_H + i16) * IDX_D + 8 * h;
#pragma unroll
    for (int hb = 0; hb < IDX_HB; ++hb) {
#pragma unroll
      for (int s = 0; s < IDX_KS; ++s) qf[k][hb * IDX_KS + s] = *reinterpret_cast<const half8_t*>(qrow + 16 * hb * IDX_D + 32 * s);
      const float* wp = wgt + (long)tok[k] * IDX_H + 16 * hb + 4 * h;
      wf[k][hb] = f32x4_t{wp[0], wp[1], wp[2], wp[3]};   // (w is 4-byte aligned only)
    }
  }

  // ---- tile staging: load n of wave w is key rows 16 n + 4 w + (lane >> 4) of the tile, a lane its 16-byte chunk lane & 15
  const int pmask = (1 << lps) - 1;
  int pid[4];
  auto page_ids = [&](int u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int first = u * IDX_KT + 16 * n;
      first = first < last ? first : last;   // (a block past the last key names the last key's page: a table position below ceil(L_b / page_size))
      int id = __builtin_amdgcn_readfirstlane(block_table[(long)b * max_pages + (first >> lps)]);
      id = id < 0 ? 0 : id;
      pid[n] = id < num_pages ? id : num_pages - 1;
    }
  };
  u32x4_t stg[4];
  auto load_tile = [&](int u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int key = u * IDX_KT + 16 * n + 4 * w + h;
      key = key < last ? key : last;
      const char* base = reinterpret_cast<const char*>(Ki) + (((long)pid[n] << lps) * (IDX_D * 2));
      stg[n] = *reinterpret_cast<const u32x4_t*>(base + ((unsigned)(key & pmask) * (IDX_D * 2) + i16 * 16));
    }
  };
  auto store_tile = [&](char* img) {
#pragma unroll
    for (int n = 0; n < 4; ++n) *reinterpret_cast<u32x4_t*>(img + (16 * n + 4 * w + h) * IDX_ROW + i16 * 16) = stg[n];
  };

  if (t1 > t0) {
    page_ids(t0);
    load_tile(t0);
    store_tile(lds);
    page_ids(t0 + 1);
  }
  __syncthreads();
  const int k_off = i16 * IDX_ROW + 16 * h;   // the fragment read: key row i16 of a 16-key block, bytes 64 s + 16 h
  for (int u = t0; u < t1; ++u) {
    const char* img = lds + ((u - t0) & 1) * IDX_TILE;
    char* nxt = lds + (((u - t0) & 1) ^ 1) * IDX_TILE;
    const bool more = u + 1 < t1;
    if (more) load_tile(u + 1);   // in flight under this tile's arithmetic
    if (wave_live) {
      for (int kb = kb0; kb < 4; kb += kstep) {
        half8_t kf[IDX_KS];
#pragma unroll
        for (int s = 0; s < IDX_KS; ++s) kf[s] = *reinterpret_cast<const half8_t*>(img + 16 * kb * IDX_ROW + k_off + 64 * s);
        const int key = u * IDX_KT + 16 * kb + i16;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (k == 1 && !two) break;
          // ---- [64 heads x 16 keys] = Qi Kᵀ: four independent chains of four k-steps
          f32x4_t acc[IDX_HB];
#pragma unroll
          for (int hb = 0; hb < IDX_HB; ++hb) acc[hb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < IDX_KS; ++s)
#pragma unroll
            for (int hb = 0; hb < IDX_HB; ++hb) acc[hb] = mfma16_16<BF16>(qf[k][hb * IDX_KS + s], kf[s], acc[hb]);
          // ---- relu, w, the sum over the lane's 16 heads, then over the four lane groups
          float sum = 0.f;
#pragma unroll
          for (int hb = 0; hb < IDX_HB; ++hb)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += wf[k][hb][e] * fmaxf(acc[hb][e], 0.f);
          sum += __shfl_xor(sum, 16);
          sum += __shfl_xor(sum, 32);
          if (h == 0 && key < nvis[k]) logits[(long)tok[k] * ld + key] = sum;   // the causal edge: a masked store
        }
      }
    }
    if (more) {
      store_tile(nxt);
      page_ids(u + 2);
    }
    __syncthreads();   // the next image is whole; every wave is done reading this one
  }
}

}  // namespace lc
