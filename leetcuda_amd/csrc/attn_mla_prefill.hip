// attn_mla_prefill.hip — the NON-ABSORBED prefill form of multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2): plain causal MHA on a
// ragged batch with scores over 192 dims and values over 128 (lc_attn_mla_prefill_f16 / _bf16).  kv_b_proj has expanded the
// latent rows into per-head Knope [Tk,H,128] and V [Tk,H,128]; the 64-wide rotated Kpe row [Tk,64] is ONE row a token, read by every head:
//   s_j = sm_scale (Q[t,h,:128] . Knope[j,h,:] + Q[t,h,128:] . Kpe[j,:]),   O[t,h,:] = sum_j softmax_j(s) V[j,h,:],   lse = ln sum_j exp(s_j)
// Queries of sequence b are tokens cu_q[b] .. cu_q[b+1] - 1, keys are rows cu_k[b] .. cu_k[b+1] - 1 (both clamped here, attn_mla.hip's clamps);
// query i sits at position Lk_b - Nq_b + i (bottom-right).  Every operand is a strided view; offsets are 64-bit.  No device code is shared
// with the decode body or with attn_mla.hip.
//
//   - work split: a workgroup (4 wave64) owns ONE head and 64 RS consecutive query tokens of one sequence; its waves split the rows, 16 RS each
//     (RS row sets of 16), and EVERY wave walks all key tiles.  Sᵀ = K Qᵀ on v_mfma_f32_16x16x32: a lane holds one query row of a set
//     (lane & 15) and 16 keys of the tile, so the softmax is lane-local and P is, register for register, the B operand of Oᵀ += Vᵀ Pᵀ.
//     Nothing is merged across waves.  Per row set: Oᵀ 128 x 16 fp32 = 32 registers, the Q fragments of 6 k-steps = 24, resident for the walk.
//     A K or V fragment read from LDS feeds the MFMAs of all RS sets: RS = 2 halves the LDS reads and the HBM / L2 tile traffic a row
//   - LDS: a 64-key tile is ONE K image of rows [128 Knope of this head | 64 Kpe] (384 + 16 bytes of padding: the six k-steps of a score are
//     ds_read_b128 along one row) and a V image of rows of 256 + 16 bytes read by ds_read_b64_tr_b16: 25 600 + 17 408 bytes, double-buffered
//     86 016.  The Kpe part comes from the shared [Tk,64] rows: they are never expanded in memory
//   - staging through registers, a tile ahead: the K part of tile u + 1 (six 16-byte loads a lane) is issued in front of the scores of tile u
//     and stored behind the softmax, the V part (four loads) is in flight under the value product; ONE barrier a tile
//   - source rows are clamped to the last walked key of the sequence and never zero-filled; a masked score is a SELECT on the key index
//     (P = 0 exactly), applied only on tiles the block's diagonal (or the end of the keys) crosses, behind one block-uniform branch
//   - grid: NB x B x H workgroups, NB = ceil(max_nq / (64 RS)).  LOGICAL order (row block DESCENDING, b, h), h fastest: the longest causal
//     walks start first, and under xcd_remap (an XCD owns a contiguous eighth) the heads of one (sequence, row block) — which read the same
//     Kpe rows — are neighbours in one L2
//   - a block whose first row is at or past Nq_b returns in front of its first barrier; a row set without a row skips the arithmetic (the
//     walk is compiled per number of live sets of the wave) but its wave keeps staging and meeting the barriers
//   - the wave normalises, rounds ONCE (RNE) and writes O and, if asked, lse (natural units); a row without a visible key: O = 0, lse = -inf
#pragma once
#include "attn_decode.hip"   // mfma16_16<BF16>, DEC_NEG_INF (lc_common.h: cvt16<BF16>, lds_tr16, cat4, xcd_remap)

namespace lc {

constexpr int MLP_DN = 128;                            // nope dims of a key (per head)
constexpr int MLP_DR = 64;                             // rope dims of a key (shared by the heads)
constexpr int MLP_DV = 128;                            // value dims
constexpr int MLP_KT = 64;                             // keys per tile
constexpr int MLP_KROW = (MLP_DN + MLP_DR) * 2 + 16;   // bytes of a row of the K image: 384 + 16 of padding
constexpr int MLP_VROW = MLP_DV * 2 + 16;              // bytes of a row of the V image: 256 + 16
constexpr int MLP_KIMG = MLP_KT * MLP_KROW;            // 25 600
constexpr int MLP_TILE = MLP_KIMG + MLP_KT * MLP_VROW; // 43 008
constexpr int MLP_LDS = 2 * MLP_TILE;                  // 86 016 of the 163 840
constexpr int MLP_KS = (MLP_DN + MLP_DR) / 32;         // 6 k-steps of a score
constexpr int MLP_DB = MLP_DV / 16;                    // 8 blocks of 16 output columns

template <bool BF16, int RS>
__global__ __launch_bounds__(256) void attn_mla_prefill_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kn,
                                                               const half_t* __restrict__ Kpe, const half_t* __restrict__ V,
                                                               half_t* __restrict__ O, float* __restrict__ lse, const int* __restrict__ cu_q,
                                                               const int* __restrict__ cu_k, int B, int H, int Tq, int Tk, int max_nq, int causal,
                                                               float sl2, long q_rs, long q_hs, long kn_rs, long kn_hs, long kpe_rs, long v_rs,
                                                               long v_hs) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int BR = 64 * RS;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, hh = lane >> 4;

  // ---- which (row block, sequence, head): logical id ((NB - 1 - rb) B + b) H + h, an XCD owning a contiguous eighth of the ids
  const int NB = __builtin_amdgcn_readfirstlane((max_nq + BR - 1) / BR);
  const int lid = __builtin_amdgcn_readfirstlane(xcd_remap((int)blockIdx.x, (int)gridDim.x));
  const int g = __builtin_amdgcn_readfirstlane(lid / H), h = lid - g * H;
  const int nbr = __builtin_amdgcn_readfirstlane(g / B), b = g - nbr * B;
  const int rbase = BR * (NB - 1 - nbr);
  const int c0 = __builtin_amdgcn_readfirstlane(cu_q[b]), c1 = __builtin_amdgcn_readfirstlane(cu_q[b + 1]);
  const int q0 = c0 < 0 ? 0 : (c0 > Tq ? Tq : c0);
  const int cap = max_nq < Tq - q0 ? max_nq : Tq - q0;
  const int Nq = c1 <= q0 ? 0 : (c1 - q0 > cap ? cap : c1 - q0);
  if (rbase >= Nq) return;   // no row of this sequence in the block (Nq_b = 0 included): nothing touched, no barrier met
  const int d0 = __builtin_amdgcn_readfirstlane(cu_k[b]), d1 = __builtin_amdgcn_readfirstlane(cu_k[b + 1]);
  const int k0 = d0 < 0 ? 0 : (d0 > Tk ? Tk : d0);
  const int Lk = d1 <= k0 ? 0 : (d1 - k0 > Tk - k0 ? Tk - k0 : d1 - k0);
  // the keys this block walks: all Lk, or (causal) those its last row sees; lim_lo: the keys its FIRST row sees — a tile that ends at or
  // below it needs no mask
  const int nrow = Nq - rbase < BR ? Nq - rbase : BR;
  int Lw = Lk, lim_lo = Lk;
  if (causal) {
    const int v = Lk - Nq + rbase + nrow;
    Lw = v < 0 ? 0 : (v > Lk ? Lk : v);
    lim_lo = Lk - Nq + rbase + 1;
    lim_lo = lim_lo < 0 ? 0 : lim_lo;
  }
  const int Tw = (Lw + MLP_KT - 1) / MLP_KT;
  const int last = Lw - 1;   // (>= 0 whenever a tile exists)

  // ---- this lane's query rows (a row >= Nq_b: row Nq_b - 1, nothing stored) and their 6 Q fragments: dims 32 s + 8 hh ... of the 192
  const int nlive = __builtin_amdgcn_readfirstlane((nrow - 16 * RS * w + 15) / 16);   // live row sets of this wave: <= 0 none, >= RS all
  int lim[RS];
  long orow[RS];
  bool owned[RS];
  half8_t qf[RS][MLP_KS];
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    const int r = rbase + 16 * (RS * w + s) + i16;
    const int rs = r < Nq ? r : Nq - 1;
    owned[s] = r < Nq;
    orow[s] = (long)(q0 + rs) * H + h;   // the row of O and lse (q0 + rs < Tq: the clamps above)
    const half_t* qp = Q + (long)(q0 + rs) * q_rs + (long)h * q_hs + 8 * hh;
#pragma unroll
    for (int k = 0; k < MLP_KS; ++k) qf[s][k] = *reinterpret_cast<const half8_t*>(qp + 32 * k);
    const int v = causal ? Lk - Nq + rs + 1 : Lk;   // keys j < lim are visible to this row
    lim[s] = v < 0 ? 0 : v;
  }

  // ---- tile staging: 16-byte chunk c = 256 n + tid.  Knope and V: row c >> 4, chunk c & 15 (n < 4); Kpe: row c >> 3, chunk c & 7 (n < 2)
  u32x4_t stg[6];
  const half_t* kn_h = Kn + (long)h * kn_hs;
  const half_t* v_h = V + (long)h * v_hs;
  auto src_row = [&](int u, int row) {
    const int key = u * MLP_KT + row;
    return (long)(k0 + (key < last ? key : last));
  };
  auto load_k = [&](int u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int c = 256 * n + tid;
      stg[n] = *reinterpret_cast<const u32x4_t*>(kn_h + src_row(u, c >> 4) * kn_rs + 8 * (c & 15));
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c = 256 * n + tid;
      stg[4 + n] = *reinterpret_cast<const u32x4_t*>(Kpe + src_row(u, c >> 3) * kpe_rs + 8 * (c & 7));
    }
  };
  auto store_k = [&](char* img) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int c = 256 * n + tid;
      *reinterpret_cast<u32x4_t*>(img + (c >> 4) * MLP_KROW + 16 * (c & 15)) = stg[n];
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int c = 256 * n + tid;
      *reinterpret_cast<u32x4_t*>(img + (c >> 3) * MLP_KROW + MLP_DN * 2 + 16 * (c & 7)) = stg[4 + n];
    }
  };
  auto load_v = [&](int u) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int c = 256 * n + tid;
      stg[n] = *reinterpret_cast<const u32x4_t*>(v_h + src_row(u, c >> 4) * v_rs + 8 * (c & 15));
    }
  };
  auto store_v = [&](char* img) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int c = 256 * n + tid;
      *reinterpret_cast<u32x4_t*>(img + MLP_KIMG + (c >> 4) * MLP_VROW + 16 * (c & 15)) = stg[n];
    }
  };

  float m[RS], l[RS];
  f32x4_t o[RS][MLP_DB];
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    m[s] = DEC_NEG_INF;
    l[s] = 0.f;
#pragma unroll
    for (int db = 0; db < MLP_DB; ++db) o[s][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // row read of the score product: key row i16 of a 16-key block, bytes 64 k + 16 hh; transposed read of the value product: rows 4 hh + q4
  // (+ 16) of a 32-key step, 8 bytes at column 16 db + 4 p4
  const int k_off = i16 * MLP_KROW + 16 * hh;
  const int tr_off = MLP_KIMG + (4 * hh + (i16 >> 2)) * MLP_VROW + 8 * (i16 & 3);

  if (Tw > 0) {
    load_k(0);
    store_k(lds);
    load_v(0);
    store_v(lds);
  }
  __syncthreads();

  // the walk, compiled for NL live row sets of the wave (0: the wave only moves data and meets the barriers)
  auto walk = [&](auto nl) {
    constexpr int NL = decltype(nl)::value;
    for (int u = 0; u < Tw; ++u) {
      char* img = lds + (u & 1) * MLP_TILE;
      char* nxt = lds + ((u & 1) ^ 1) * MLP_TILE;
      const bool more = u + 1 < Tw;
      // the K part of the next tile, in flight under this tile's scores
      if (more) load_k(u + 1);
      if constexpr (NL == 0) {
        if (more) {
          store_k(nxt);
          load_v(u + 1);
          store_v(nxt);
        }
      } else {
        // ---- Sᵀ = K Qᵀ: four 16-key blocks x 6 k-steps (the rope dims last); a K fragment serves every live row set
        f32x4_t st[NL][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
          for (int s = 0; s < NL; ++s) st[s][kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < MLP_KS; ++k) {
            const half8_t ka = *reinterpret_cast<const half8_t*>(img + 16 * kb * MLP_KROW + k_off + 64 * k);
#pragma unroll
            for (int s = 0; s < NL; ++s) st[s][kb] = mfma16_16<BF16>(ka, qf[s][k], st[s][kb]);
          }
        }
        // ---- online softmax in the log2 domain; register e of block kb is key 64 u + 16 kb + 4 hh + e.  The select on the key INDEX runs
        // only on a tile that reaches past the keys the block's first row sees (block-uniform)
        const int kfirst = u * MLP_KT + 4 * hh;
        const bool masked = (u + 1) * MLP_KT > lim_lo;
        half8_t pf[NL][2];
        float alpha[NL];
#pragma unroll
        for (int s = 0; s < NL; ++s) {
          float mx = DEC_NEG_INF;
          if (masked) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float x = kfirst + 16 * kb + e < lim[s] ? st[s][kb][e] * sl2 : DEC_NEG_INF;   // the score may be anything
                st[s][kb][e] = x;
                mx = fmaxf(mx, x);
              }
          } else {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float x = st[s][kb][e] * sl2;
                st[s][kb][e] = x;
                mx = fmaxf(mx, x);
              }
          }
          mx = fmaxf(mx, __shfl_xor(mx, 16));
          mx = fmaxf(mx, __shfl_xor(mx, 32));
          const float mn = fmaxf(m[s], mx);
          const float mu = (mn == DEC_NEG_INF) ? 0.f : mn;   // no visible key yet: every exponent below is exp2(-inf) = 0
          alpha[s] = __builtin_amdgcn_exp2f(m[s] - mu);
          m[s] = mn;
          float ps = 0.f;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float p = __builtin_amdgcn_exp2f(st[s][kb][e] - mu);
              ps += p;   // (the row sum keeps the unrounded value)
              pf[s][kb >> 1][4 * (kb & 1) + e] = cvt16<BF16>(p);
            }
          l[s] = l[s] * alpha[s] + ps;
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- the next K image, and the V part of the next tile in flight under the value product
        if (more) {
          store_k(nxt);
          load_v(u + 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- rescale Oᵀ only when some row's maximum moved (a multiplication by exactly 1 otherwise: same bits)
#pragma unroll
        for (int s = 0; s < NL; ++s)
          if (__builtin_amdgcn_ballot_w64(alpha[s] != 1.f) != 0) {
#pragma unroll
            for (int db = 0; db < MLP_DB; ++db) o[s][db] *= alpha[s];
          }
        // ---- Oᵀ += Vᵀ Pᵀ: a transposed V fragment serves every live row set
#pragma unroll
        for (int db = 0; db < MLP_DB; ++db) {
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const half8_t va = cat4(lds_tr16(img + (32 * t) * MLP_VROW + tr_off + 32 * db), lds_tr16(img + (32 * t + 16) * MLP_VROW + tr_off + 32 * db));
#pragma unroll
            for (int s = 0; s < NL; ++s) o[s][db] = mfma16_16<BF16>(va, pf[s][t], o[s][db]);
          }
        }
        if (more) store_v(nxt);
      }
      __syncthreads();   // the next images are whole; every wave is done reading these
    }
  };
  if (nlive <= 0) {
    walk(std::integral_constant<int, 0>{});
    return;
  }
  if constexpr (RS == 2) {
    if (nlive == 1) walk(std::integral_constant<int, 1>{});
    else walk(std::integral_constant<int, 2>{});
  } else {
    walk(std::integral_constant<int, 1>{});
  }

  // ---- a wave owns its rows: no merge across waves.  The four lane groups of a row hold disjoint keys: sum l once
#pragma unroll
  for (int s = 0; s < RS; ++s) {
    if (!owned[s]) continue;
    float ls = l[s];
    ls += __shfl_xor(ls, 16);
    ls += __shfl_xor(ls, 32);
    const float inv = ls > 0.f ? 1.f / ls : 0.f;
    half_t* dst = O + orow[s] * MLP_DV + 4 * hh;
#pragma unroll
    for (int db = 0; db < MLP_DB; ++db) {
      const f32x4_t x = o[s][db] * inv;
      const half4_t y = {cvt16<BF16>(x[0]), cvt16<BF16>(x[1]), cvt16<BF16>(x[2]), cvt16<BF16>(x[3])};
      *reinterpret_cast<half4_t*>(dst + 16 * db) = y;
    }
    if (lse && hh == 0) lse[orow[s]] = ls > 0.f ? (m[s] + log2f(ls)) * 0.6931471805599453f : DEC_NEG_INF;
  }
}

}  // namespace lc
