// attn_decode.hip — decode attention over a KV cache (lc_attn_decode_f16): Nq new query tokens per sequence, G = H / Hkv
// query heads per K / V head, R = G x Nq <= 64 query rows per (batch, K / V head) against L_b = kv_len[b] cached keys.
//
// The problem is bound by reading K and V ONCE from HBM, so nothing here is shared between waves and nothing is read twice:
//   - one workgroup (4 wave64) per (batch, K / V head, KV range s of S); the range partition is computed IN THE KERNEL from L_b
//     (T_b = ceil(L_b / 64) tiles, range s = tiles [s T_b / S, (s + 1) T_b / S)): the host never sees kv_len, a range may be empty
//   - wave w owns the 64-key tiles t0 + w, t0 + w + 4, ... of the range and keeps its own online softmax (running max, sum, fp32 O); there is
//     no workgroup barrier inside the key loop, and ONE merge of the four (m, l, O) through LDS behind it
//   - K goes straight from global memory into MFMA-operand registers: Sᵀ = K Qᵀ on v_mfma_f32_16x16x32_f16 with the K rows as the A operand;
//     lane (key = lane & 15, h = lane >> 4) reads the D / 4 CONTIGUOUS halves d = h D / 4 ... of its key row (64 bytes at D = 128) and k-step s
//     takes elements 8 s ... 8 s + 7 of them — Q is read from its LDS image under the same permutation of d, so the sum is over every d once
//   - Sᵀ leaves each lane with ONE query row (lane & 15) and 16 keys of the tile: P in fp16 is, register for register, the B operand of
//     Oᵀ = Vᵀ Pᵀ (no shuffle); the A operand Vᵀ comes from a per-wave row-major LDS image of the V tile through ds_read_b64_tr_b16.  The next
//     tile's K and V loads are issued (into registers) behind the current tile's softmax, and V is copied to the image at the end of the
//     iteration: the loads of a whole tile (32 KiB at D = 128) are in flight per wave while it computes
//   - masking is a SELECT on the key index before the row maximum (a score may be NaN); K / V source rows are clamped to <= L_b - 1 and never
//     zero-filled, so a masked P = 0 never meets a NaN of the cache tail and every address stays inside [0, Ncap) (the rule of §4.2c)
//   - rows R ... 16 RT - 1 of the padded row tiles load Q row R - 1 and store nothing
//   - S == 1: the workgroup normalises and writes fp16 O.  S > 1: it writes the NORMALISED fp32 partial O and the row's log-sum-exp in the
//     log2 domain (-inf: the range held no visible key) to the workspace; attn_decode_combine_kernel<D> merges the S partials (weight 0 for
//     an empty range, O = 0 when every range is empty)
// Reproducibility: the bits of one (batch, K / V head) depend on its Q, K, V, L_b, Nq, the causal flag and S only.
#pragma once
#include "lc_common.h"

namespace lc {

constexpr int DEC_KVB = 64;      // keys per tile
constexpr int DEC_WAVES = 4;
constexpr float DEC_NEG_INF = -__builtin_inff();

// byte offset of 16-byte chunk `ch` of key row `row` in the per-wave V image (rows of D halves, chunks XOR-swizzled by the row so that the
// four rows of a transposed 4 x 16 block read fall on different banks)
template <int D>
LC_DEVINL int dec_v_off(int row, int ch) {
  if constexpr (D == 128) return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  else return 128 * row + 16 * (ch ^ (((row & 3) << 1) | ((row >> 2) & 1)));
}

template <int D, int RT>
struct DecodeLds {
  static constexpr int kQStride = D * 2 + 16;                  // bytes per Q row: 16 bytes of padding spread the 16 rows of a fragment read over the banks
  static constexpr int kQBytes = 16 * RT * kQStride;
  static constexpr int kVBytes = DEC_KVB * D * 2;              // one wave's V image (a step of 64 keys; the merge slots need it whole)
  static constexpr int kOBytes = RT * (D / 16) * 4 * 64 * 4;   // one wave's O accumulators (merge)
  static constexpr int kMlOff = kQBytes;                       // m[4][16 RT], l[4][16 RT]
  static constexpr int kMlBytes = 2 * DEC_WAVES * 16 * RT * 4;
  static constexpr int kVOff = kMlOff + kMlBytes;
  static constexpr int kTotal = kVOff + DEC_WAVES * kVBytes;   // (the merge re-uses the V images: two slots of kOBytes <= 4 kVBytes)
  static_assert(2 * kOBytes <= DEC_WAVES * kVBytes, "merge slots must fit the V images");
};

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
                                                          half_t* __restrict__ O, const int* __restrict__ kv_len, float* __restrict__ part_o,
                                                          float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap, int causal, int S,
                                                          float sl2, long total_rows) {
  using L = DecodeLds<D, RT>;
  constexpr int KS = D / 32;    // k-steps of Sᵀ = K Qᵀ
  constexpr int DB = D / 16;    // 16-wide blocks of d
  constexpr int CH = D / 8;     // 16-byte chunks per row
  // keys per pipeline step: a wave walks its 64-key tiles in steps of 64 keys — of 32 where the accumulators of four row tiles at D = 128 leave
  // no room for a whole tile's K and V in flight (hipcc spilled; the audit's rule R2)
  constexpr int STEP = (D == 128 && RT == 4) ? 32 : 64;
  constexpr int SPT = DEC_KVB / STEP;     // steps per tile
  constexpr int NKB = STEP / 16;          // 16-key blocks of Sᵀ per step
  constexpr int NPS = STEP / 32;          // 32-key k-steps of Oᵀ += Vᵀ Pᵀ per step
  constexpr int VL = STEP * CH / 64;      // V chunks per lane and step
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;
  // (integer division runs on the vector ALU: readfirstlane tells hipcc that the quotients are wave-uniform — scalar addressing, a scalar tile loop)
  const int bk = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)S)), s_idx = (int)blockIdx.x - bk * S;
  const int b = __builtin_amdgcn_readfirstlane(bk / Hkv), kvh = bk - b * Hkv;
  const int G = __builtin_amdgcn_readfirstlane(H / Hkv), R = G * Nq;
  int Lb = kv_len ? kv_len[b] : Ncap;
  Lb = __builtin_amdgcn_readfirstlane(Lb);   // (a vector load of a uniform address: tell hipcc that the tile loop is wave-uniform)
  Lb = Lb < 0 ? 0 : (Lb > Ncap ? Ncap : Lb);
  const int T = (Lb + DEC_KVB - 1) / DEC_KVB;
  // (T < 2^24 tiles — one head's cache is below 2 GiB — and S <= 64: the products fit 32 bits)
  const int t0 = __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * T) / (unsigned)S));
  const int t1 = __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * T) / (unsigned)S));

  const long row0 = ((long)b * H + (long)kvh * G) * Nq;   // the R rows of this (batch, K / V head): one contiguous [R, D] matrix
  const half_t* Qg = Q + row0 * D;
  const half_t* Kg = K + ((long)b * Hkv + kvh) * (long)Ncap * D;
  const half_t* Vg = V + ((long)b * Hkv + kvh) * (long)Ncap * D;

  // ---- Q -> LDS (rows >= R: row R - 1)
  for (int c = tid; c < 16 * RT * CH; c += 256) {
    const int r = c / CH, ch = c % CH;
    const int rs = r < R ? r : R - 1;
    *reinterpret_cast<u32x4_t*>(lds + r * L::kQStride + ch * 16) = *reinterpret_cast<const u32x4_t*>(Qg + (long)rs * D + ch * 8);
  }
  __syncthreads();

  // visible keys of this lane's query row in each row tile: keys j < lim
  int lim[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    int r = 16 * rt + i16;
    r = r < R ? r : R - 1;
    int v = causal ? Lb - Nq + (r % Nq) + 1 : Lb;
    lim[rt] = v < 0 ? 0 : v;
  }

  float m[RT], l[RT];
  f32x4_t o[RT][DB];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    m[rt] = DEC_NEG_INF;
    l[rt] = 0.f;
#pragma unroll
    for (int db = 0; db < DB; ++db) o[rt][db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  char* vimg = lds + L::kVOff + w * L::kVBytes;
  // transposed-read address of this lane inside a 32-key k-step: row 4 h + q (+ 16 for the second half), d = 16 db + 4 p
  const int q4 = i16 >> 2, p4 = i16 & 3;
  int tr_off[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) tr_off[db] = dec_v_off<D>(4 * h + q4, 2 * db + (p4 >> 1)) + 8 * (p4 & 1);

  u32x4_t kf[NKB][KS], vf[VL];
  const int last = Lb - 1;   // (>= 0 whenever a tile exists)
  // step u of this wave: keys key0(u) ... key0(u) + STEP - 1 of tile t0 + w + 4 (u / SPT)
  auto key0 = [&](int u) { return (t0 + w + DEC_WAVES * (u / SPT)) * DEC_KVB + (u % SPT) * STEP; };
  auto load_k = [&](int u) {
    const int k0 = key0(u);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      int key = k0 + 16 * kb + i16;
      key = key < last ? key : last;
      const unsigned off = (unsigned)key * (D * 2) + h * (D / 2);   // bytes inside the head: < 2 GiB (checked by the host), base in SGPRs
#pragma unroll
      for (int s = 0; s < KS; ++s) kf[kb][s] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(Kg) + (off + 16 * s));
    }
  };
  auto load_v = [&](int u) {
    const int k0 = key0(u);
#pragma unroll
    for (int n = 0; n < VL; ++n) {
      const int c = n * 64 + lane;
      int key = k0 + c / CH;
      key = key < last ? key : last;
      vf[n] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(Vg) + ((unsigned)key * (D * 2) + (c % CH) * 16));
    }
  };
  auto store_v = [&]() {
#pragma unroll
    for (int n = 0; n < VL; ++n) {
      const int c = n * 64 + lane;
      *reinterpret_cast<u32x4_t*>(vimg + dec_v_off<D>(c / CH, c % CH)) = vf[n];
    }
  };

  const int my_tiles = t1 - t0 - w > 0 ? (t1 - t0 - w + DEC_WAVES - 1) / DEC_WAVES : 0;
  const int steps = my_tiles * SPT;
  if (steps > 0) {
    load_k(0);
    load_v(0);
    store_v();
  }
  for (int u = 0; u < steps; ++u) {
    // ---- Sᵀ = K Qᵀ for this tile (the K registers are free behind it)
    // and the online softmax (log2 domain) of each row tile right behind its scores: Sᵀ -> P in fp16, register for register the B operand of
    // Oᵀ += Vᵀ Pᵀ (16 score registers per lane alive at a time, not 16 RT)
    const int k0 = key0(u) + 4 * h;
    half8_t pf[RT][NPS];
    float alpha[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      half8_t qf[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s)
        qf[s] = *reinterpret_cast<const half8_t*>(lds + (16 * rt + i16) * L::kQStride + (h * (D / 4) + 8 * s) * 2);
      f32x4_t st[NKB];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma16(__builtin_bit_cast(half8_t, kf[kb][s]), qf[s], acc);
        st[kb] = acc;
      }
      float mx = DEC_NEG_INF;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = (k0 + 16 * kb + r < lim[rt]) ? st[kb][r] * sl2 : DEC_NEG_INF;   // select on the INDEX: the score may be anything
          st[kb][r] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m[rt], mx);
      const float mu = (mn == DEC_NEG_INF) ? 0.f : mn;   // no visible key yet: every exponent below is exp2(-inf) = 0
      alpha[rt] = __builtin_amdgcn_exp2f(m[rt] - mu);
      m[rt] = mn;
      float ps = 0.f;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(st[kb][r] - mu);
          ps += p;
          pf[rt][kb >> 1][4 * (kb & 1) + r] = (half_t)p;
        }
      l[rt] = l[rt] * alpha[rt] + ps;   // (this lane's keys of the step: the four lane groups of a row are summed once, behind the loop)
    }
    // ---- the next tile's K and V loads into the registers that are free now: a whole tile in flight under the rest of the arithmetic (the
    // scheduling barrier keeps hipcc from hoisting them over the scores: that is what keeps the four-row-tile kernel inside the register file)
    __builtin_amdgcn_sched_barrier(0);
    const bool more = u + 1 < steps;
    if (more) load_k(u + 1);
    if (more) load_v(u + 1);
    // ---- rescale O only when some row's maximum moved (a multiplication by exactly 1 otherwise: same bits).  A block of its own, so that the
    // accumulators stay where the MFMAs below want them instead of travelling through the vector ALU on every tile
    bool moved = false;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) moved |= alpha[rt] != 1.f;
    if (__builtin_amdgcn_ballot_w64(moved) != 0) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int db = 0; db < DB; ++db) o[rt][db] *= alpha[rt];
    }
    // ---- Oᵀ += Vᵀ Pᵀ: the Vᵀ fragments of a 16-wide block of d out of the image serve every row tile
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      half8_t va[NPS];
#pragma unroll
      for (int s = 0; s < NPS; ++s) va[s] = cat4(lds_tr16(vimg + (D * 2) * (32 * s) + tr_off[db]), lds_tr16(vimg + (D * 2) * (32 * s + 16) + tr_off[db]));
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int s = 0; s < NPS; ++s) o[rt][db] = mfma16(va[s], pf[rt][s], o[rt][db]);
    }
    if (more) store_v();   // (LDS operations of one wave execute in order: the transposed reads above are behind us)
  }

  // ---- merge the four waves' (m, l, O)
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    l[rt] += __shfl_xor(l[rt], 16);
    l[rt] += __shfl_xor(l[rt], 32);
  }
  float* ml = reinterpret_cast<float*>(lds + L::kMlOff);
  if (h == 0) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      ml[w * 16 * RT + 16 * rt + i16] = m[rt];
      ml[(DEC_WAVES + w) * 16 * RT + 16 * rt + i16] = l[rt];
    }
  }
  __syncthreads();   // every wave is out of its key loop: the V images are free
  float lt[RT], mt[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float mm = DEC_NEG_INF;
#pragma unroll
    for (int x = 0; x < DEC_WAVES; ++x) mm = fmaxf(mm, ml[x * 16 * RT + 16 * rt + i16]);
    const float mu = (mm == DEC_NEG_INF) ? 0.f : mm;
    float ls = 0.f;
#pragma unroll
    for (int x = 0; x < DEC_WAVES; ++x) ls += ml[(DEC_WAVES + x) * 16 * RT + 16 * rt + i16] * __builtin_amdgcn_exp2f(ml[x * 16 * RT + 16 * rt + i16] - mu);
    const float mine = __builtin_amdgcn_exp2f(m[rt] - mu);
#pragma unroll
    for (int db = 0; db < DB; ++db) o[rt][db] *= mine;
    lt[rt] = ls;
    mt[rt] = mm;
  }
  f32x4_t* slot = reinterpret_cast<f32x4_t*>(lds + L::kVOff);
  constexpr int SLOT = L::kOBytes / 16;   // f32x4 per slot
  auto put = [&](int sl) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int db = 0; db < DB; ++db) slot[sl * SLOT + (rt * DB + db) * 64 + lane] = o[rt][db];
  };
  auto add = [&](int sl) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int db = 0; db < DB; ++db) o[rt][db] += slot[sl * SLOT + (rt * DB + db) * 64 + lane];
  };
  if (w >= 2) put(w - 2);
  __syncthreads();
  if (w < 2) add(w);
  __syncthreads();
  if (w == 1) put(0);
  __syncthreads();
  if (w != 0) return;
  add(0);

  // ---- wave 0 writes: fp16 O (S == 1) or the normalised fp32 partial + the row's log2-domain log-sum-exp
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = 16 * rt + i16;
    if (r >= R) continue;   // padding rows store nothing
    const float inv = lt[rt] > 0.f ? 1.f / lt[rt] : 0.f;
    const long row = row0 + r;
    if (S == 1) {
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const f32x4_t x = o[rt][db] * inv;
        half4_t y = {(half_t)x[0], (half_t)x[1], (half_t)x[2], (half_t)x[3]};
        *reinterpret_cast<half4_t*>(O + row * D + 16 * db + 4 * h) = y;
      }
    } else {
      float* po = part_o + ((long)s_idx * total_rows + row) * D;
#pragma unroll
      for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4_t*>(po + 16 * db + 4 * h) = o[rt][db] * inv;
      if (h == 0) part_lse[(long)s_idx * total_rows + row] = lt[rt] > 0.f ? mt[rt] + log2f(lt[rt]) : DEC_NEG_INF;
    }
  }
}

// O[row] = sum_s w_s part_o[s][row] / sum_s w_s with w_s = exp2(lse_s - max lse): weight 0 for a range without a visible key (lse = -inf),
// O = 0 when no range has one.  One thread per (row, four d).
template <int D>
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                  half_t* __restrict__ O, long total_rows, int S) {
  constexpr int TPR = D / 4;   // threads per row
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
      if (wgt > 0.f) {   // (an empty range's partial is 0, but it is never read: weight 0 is not a multiplication)
        acc += *reinterpret_cast<const f32x4_t*>(part_o + ((long)s * total_rows + row) * D + d) * wgt;
        ws += wgt;
      }
    }
  }
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  half4_t y = {(half_t)(acc[0] * inv), (half_t)(acc[1] * inv), (half_t)(acc[2] * inv), (half_t)(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * D + d) = y;
}

}  // namespace lc
