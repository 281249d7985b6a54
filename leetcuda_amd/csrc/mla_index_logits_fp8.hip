// mla_index_logits_fp8.hip — the index logits of the lightning indexer over an fp8 (OCP e4m3fn) PAGED index-key pool with per-row scales
// (lc_mla_index_logits_fp8): for query token t of sequence b and visible key position j, s = slot(b, j),
//   logit[t, j] = ks[s] · sum_{h < 64} w[t, h] · max(0, sum_{d < 128} q8[t, h, d] · k8[s, d])
// q8 [T,64,128] and k8 [num_pages, page_size, 128] are e4m3fn codes, ks [num_pages, page_size] fp32 (a pool of its own: key rows keep their
// 16-byte alignment), w [T,64] fp32 with every query-side scale folded in.  THE ORDER, which a reference can follow: the 128 products of UNSCALED
// codes are summed by the MFMA (fp32 result), max(., 0) on that sum, ONE fp32 multiply by w[t, h] accumulated over the 64 heads (head blocks
// ascending inside a lane, then lane groups +16, +32), then ONE fp32 multiply by ks[s].  Every other rule — the ragged batch, visibility, exactly
// the columns [0, n_t) written, clamped source rows and page ids — is mla_index_logits.hip's (§4.3u), word for word.
//
//   - the product: v_mfma_scale_f32_16x16x128_f8f6f4, both formats e4m3, both block scales 2^0 (E8M0 0x7f), consumes the WHOLE Di = 128 of a
//     16-head x 16-key block in one issue: four independent MFMAs with a zero C per (token, 16 keys), where the 16-bit kernel chains 16.  q8 is
//     the ROW operand, the key block the column operand: a lane ends up with ONE key (lane & 15) and the heads 16 hb + 4 (lane >> 4) + e, so
//     relu, w and the sum over its 16 heads are lane-local, the sum over the lane groups two cross-lane steps, the multiply by ks one more
//     lane-local instruction behind them.  A lane's 32 operand bytes are bytes 16 g .. + 15 and 64 + 16 g .. + 15 (g = lane >> 4) of its row —
//     the hardware's k-assignment (gemm_fp8_w4k.hip), though all that matters is that both operands use the same one
//   - registers: a token's q8 is 4 operands = 32 VGPRs and its w 16.  A wave owns TPW tokens: TPW = 4 (a workgroup 16 tokens: a prefill chunk
//     reads a key tile once per 16 tokens) or TPW = 2 (8 tokens; 96 instead of 192 registers of Q and w).  The host picks (lc_plan.h): 2 when
//     max_nq <= 8 — no block then holds a third token for a wave, and the smaller kernel keeps more workgroups and so more key bytes in flight
//     on a CU —, else 4.  One scheme for both, §4.3u's: the block's tokens form ng = ceil(nt / TPW) groups; with npp = ng rounded up to 1, 2 or 4
//     wave w owns group w % npp and the 16-key blocks w / npp, w / npp + 4 / npp, ... of the tile's eight
//   - tiles: 128 keys = 16 KiB of codes (the bytes in flight per workgroup of the 16-bit kernel's 64-key tile), LDS rows of 128 + 16 bytes,
//     double-buffered: 36 864 bytes.  Four 16-byte loads a lane a tile — load n of wave w is rows 32 n + 8 w + (lane >> 3), chunk lane & 7 —
//     issued in front of the tile's arithmetic and stored behind it; ONE barrier a tile.  A 16-key block never straddles a page, so the page
//     id of a load is a scalar load a tile ahead and its 64-bit bases live in SGPRs
//   - the scales travel THROUGH LDS, in the first four padding bytes of their key's row: the staging lane of chunk 0 loads its row's scale off
//     the same scalar page base and stores it behind the codes.  No LDS beyond the image, one ds_read_b32 a key block (row stride 36 dwords: 16
//     distinct banks), and the arithmetic never waits on a global load of its own — a lane-local load in the key-block loop would need the
//     page ids of the CURRENT tile, which the SGPRs have given up to the next one by then
//   - grid B x NB x S, NB = ceil(max_nq / (4 TPW)), logical order (b, s, nb) under xcd_remap, the S ranges of the 128-key tiles, the masked
//     store at the causal edge and the early return of an empty block: §4.3u
// Builtins and plain HIP only; every store is an ordinary vector store.
#pragma once
#include "lc_common.h"

namespace lc {

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));

constexpr int IDX8_H = 64;                        // index heads
constexpr int IDX8_D = 128;                       // index head dim = bytes of a key row
constexpr int IDX8_KT = 128;                      // keys per tile
constexpr int IDX8_ROW = IDX8_D + 16;             // bytes of a key row in the LDS image; bytes 128 .. 131: the row's scale
constexpr int IDX8_TILE = IDX8_KT * IDX8_ROW;     // 18 432 bytes
constexpr int IDX8_LDS = 2 * IDX8_TILE;           // 36 864 of the 163 840
constexpr int IDX8_HB = IDX8_H / 16;              // 4 head blocks
constexpr int IDX8_KB = IDX8_KT / 16;             // 8 key blocks a tile

// [16 heads x 16 keys] += q8 k8ᵀ over all 128 dims: formats 0 = e4m3, scales 2^0
LC_DEVINL f32x4_t mfma16_fp8_k128(i32x8_t q, i32x8_t k, f32x4_t c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(q, k, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}
// a lane's operand: bytes 16 g .. + 15 and 64 + 16 g .. + 15 of its row (p points at byte 16 g)
LC_DEVINL i32x8_t idx8_operand(const char* p) {
  const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(p), hi = *reinterpret_cast<const i32x4_t*>(p + 64);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int TPW>
__global__ __launch_bounds__(256) void mla_index_logits_fp8_kernel(const uint8_t* __restrict__ Q8, const float* __restrict__ wgt,
                                                                   const uint8_t* __restrict__ K8, const float* __restrict__ Ks,
                                                                   float* __restrict__ logits, const int* __restrict__ cu_q,
                                                                   const int* __restrict__ block_table, const int* __restrict__ kv_len, int T,
                                                                   int max_nq, int num_pages, int lps, int max_pages, int causal, int S, int NB,
                                                                   long ld) {
  constexpr int TB = 4 * TPW;   // query tokens per workgroup
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
  const int ib = nb * TB;   // the block's first token of the sequence
  if (ib >= Nqb) return;    // no token of this sequence in the block (Nq_b = 0 included): nothing touched, no barrier met
  const int Ncap = max_pages << lps;
  int Lb = __builtin_amdgcn_readfirstlane(kv_len[b]);
  Lb = Lb < 0 ? 0 : (Lb > Ncap ? Ncap : Lb);
  const int nt = Nqb - ib < TB ? Nqb - ib : TB;   // tokens of the block: 1 .. TB
  // keys j < n(i) are visible to token i of the sequence; the block walks those of its last token
  auto visible = [&](int i) {
    const int v = causal ? Lb - Nqb + i + 1 : Lb;
    return v < 0 ? 0 : (v > Lb ? Lb : v);
  };
  const int Lw = visible(ib + nt - 1);
  const int Tw = (Lw + IDX8_KT - 1) / IDX8_KT;
  const int t0 = __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * Tw) / (unsigned)S));
  const int t1 = __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * Tw) / (unsigned)S));
  const int last = Lw - 1;   // (>= 0 whenever a tile exists)

  // ---- the wave's group of tokens and its 16-key blocks of a tile (all wave-uniform)
  const int ng = (nt + TPW - 1) / TPW;
  const int npp = ng == 1 ? 1 : (ng == 2 ? 2 : 4);
  const int grp = w & (npp - 1), kb0 = w / npp, kstep = 4 / npp;
  const bool wave_live = grp < ng;                                    // (ng = 3: the fourth wave only moves data)
  const int ia = ib + TPW * (wave_live ? grp : 0);                    // the group's first token
  const int ntok = !wave_live ? 0 : (ib + nt - ia < TPW ? ib + nt - ia : TPW);   // its tokens: 1 .. TPW
  int tok[TPW], nvis[TPW];
#pragma unroll
  for (int k = 0; k < TPW; ++k) {
    tok[k] = q0 + (k < ntok ? ia + k : ia);                           // (< T: the clamps above)
    nvis[k] = k < ntok ? visible(ia + k) : 0;
  }

  // ---- Q operands of the group: head 16 hb + i16, bytes 16 h .. and 64 + 16 h ..; w: heads 16 hb + 4 h + e
  i32x8_t qf[TPW][IDX8_HB];
  f32x4_t wf[TPW][IDX8_HB];
#pragma unroll
  for (int k = 0; k < TPW; ++k) {
    const char* qrow = reinterpret_cast<const char*>(Q8) + ((long)tok[k] * IDX8_H + i16) * IDX8_D + 16 * h;
#pragma unroll
    for (int hb = 0; hb < IDX8_HB; ++hb) {
      qf[k][hb] = idx8_operand(qrow + 16 * hb * IDX8_D);
      const float* wp = wgt + (long)tok[k] * IDX8_H + 16 * hb + 4 * h;
      wf[k][hb] = f32x4_t{wp[0], wp[1], wp[2], wp[3]};   // (w is 4-byte aligned only)
    }
  }

  // ---- tile staging: load n of wave w is key rows 32 n + 8 w + (lane >> 3) of the tile, a lane its 16-byte chunk lane & 7; the row's
  // scale comes with chunk 0.  The 16-key block of a load, 2 n + (w >> 1), names its page
  const int pmask = (1 << lps) - 1;
  const int srow = 8 * w + (lane >> 3), chunk = lane & 7;
  int pid[4];
  auto page_ids = [&](int u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int first = u * IDX8_KT + 32 * n + 16 * (w >> 1);
      first = first < last ? first : last;   // (a block past the last key names the last key's page: a table position below ceil(L_b / page_size))
      int id = __builtin_amdgcn_readfirstlane(block_table[(long)b * max_pages + (first >> lps)]);
      id = id < 0 ? 0 : id;
      pid[n] = id < num_pages ? id : num_pages - 1;
    }
  };
  u32x4_t stg[4];
  float scl[4];
  auto load_tile = [&](int u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int key = u * IDX8_KT + 32 * n + srow;
      key = key < last ? key : last;
      const long slot0 = (long)pid[n] << lps;   // the page's first slot: scalar
      const unsigned off = (unsigned)(key & pmask);
      stg[n] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(K8) + slot0 * IDX8_D + (off * IDX8_D + chunk * 16));
      scl[n] = (Ks + slot0)[off];   // (the eight lanes of a row name one address)
    }
  };
  auto store_tile = [&](char* img) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      char* row = img + (32 * n + srow) * IDX8_ROW;
      *reinterpret_cast<u32x4_t*>(row + chunk * 16) = stg[n];
      if (chunk == 0) *reinterpret_cast<float*>(row + IDX8_D) = scl[n];
    }
  };

  if (t1 > t0) {
    page_ids(t0);
    load_tile(t0);
    store_tile(lds);
    page_ids(t0 + 1);
  }
  __syncthreads();
  const int k_off = i16 * IDX8_ROW + 16 * h;   // the operand read: key row i16 of a 16-key block, bytes 16 h .. and 64 + 16 h ..
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  for (int u = t0; u < t1; ++u) {
    const char* img = lds + ((u - t0) & 1) * IDX8_TILE;
    char* nxt = lds + (((u - t0) & 1) ^ 1) * IDX8_TILE;
    const bool more = u + 1 < t1;
    if (more) load_tile(u + 1);   // in flight under this tile's arithmetic
    if (wave_live) {
      for (int kb = kb0; kb < IDX8_KB; kb += kstep) {
        const char* blk = img + 16 * kb * IDX8_ROW;
        const i32x8_t kf = idx8_operand(blk + k_off);
        const float ksc = *reinterpret_cast<const float*>(blk + i16 * IDX8_ROW + IDX8_D);
        const int key = u * IDX8_KT + 16 * kb + i16;
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
          if (k < ntok) {   // (wave-uniform: a lone token pays no second product)
            // ---- [64 heads x 16 keys] = q8 k8ᵀ: four independent MFMAs
            f32x4_t acc[IDX8_HB];
#pragma unroll
            for (int hb = 0; hb < IDX8_HB; ++hb) acc[hb] = mfma16_fp8_k128(qf[k][hb], kf, zero);
            // ---- relu, w, the sum over the lane's 16 heads, then over the four lane groups; the key's scale last
            float sum = 0.f;
#pragma unroll
            for (int hb = 0; hb < IDX8_HB; ++hb)
#pragma unroll
              for (int e = 0; e < 4; ++e) sum += wf[k][hb][e] * fmaxf(acc[hb][e], 0.f);
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            if (h == 0 && key < nvis[k]) logits[(long)tok[k] * ld + key] = sum * ksc;   // the causal edge: a masked store
          }
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
