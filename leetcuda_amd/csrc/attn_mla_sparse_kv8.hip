// attn_mla_sparse_kv8.hip — SPARSE multi-head latent attention over an fp8 (e4m3fn) latent pool: every query token attends to its own `topk`
// selected slots of the pool lc_mla_append_paged_kv8 writes (lc_attn_mla_sparse_kv8 / _kv8_bf16).  CKV is [num_slots, 512]
// code bytes, an element's value is code x ckv_scale[0]; KPE stays 16-bit in the element type of Q.  A key is 640 gathered bytes instead of 1152.
//
// From attn_mla_sparse_kernel (§4.3t): the grid T x RB x S under xcd_remap, four waves of 16 heads, the 18 Q fragments, the one LDS image read by
// rows for the scores and transposed for the values and its double buffer, the lane-local softmax, the validity ballot as the ONLY mask, and the
// S > 1 partials merged by the unchanged attn_mla_sparse_combine_kernel<BF16>.  From attn_mla_paged_kv8_kernel (§4.3r): codes are converted
// once at staging with kv8_16x8<BF16>, so the image is byte for byte the 16-bit one built from the unscaled code values; the scale is applied
// in fp32, to a score chain between its 16 latent and its 2 rope k-steps and in the epilogue behind 1 / l; it is read once per workgroup by the
// kernel (NULL: 1.0), so a replayed graph sees a new scale.  What is this kernel's own:
//   - a WHOLE tile per round trip: wave w stages rows 16 w .. 16 w + 15 of the tile, latent AND rope part (one wave answers for a row), which
//     is eight 16-byte loads of codes and two of rope halves a lane, 40 VGPRs.  All ten of tile u + 1 are issued at the top of tile u, in front
//     of the scores, and converted and stored into the other image behind the value product, in front of the tile's one barrier.  So the
//     entries of tile u + 1 are in registers at the top of tile u: the 256-byte entry fetch runs TWO tiles ahead (issued at the top of tile u
//     for tile u + 2, in front of the pool loads), and the validity mask of tile u + 1 is an SGPR pair from the top of tile u to its store
//   - a 1 KiB load instruction covers TWO gathered rows: code load n of wave w is rows 16 w + 2 n + (lane >> 5), chunk lane & 31 (16 codes).
//     The two slots are unrelated, so the base is per HALF-wave and lives in VGPRs: two v_readlane of the clamped entries and one select on
//     lane >> 5 a load; the offset slot x 512 is 64-bit (num_slots x 512 may pass 2 GiB).  The rope loads keep the 16-bit kernel's map (rows
//     16 w + 8 n + (lane >> 3), chunk lane & 7, the slot through ds_bpermute)
//   - an INVALID entry is clamped to slot 0 once per tile (in bounds, never used); what reaches LDS is a select on the entry's mask bit between
//     the converted registers and ZERO, never a function of pool data (codes 0x7f / 0xff are NaN).  A wave whose 16 entries are all invalid
//     issues no pool load at all: a tile of -1 padding moves no pool data
// The score / softmax / value block is stated again here rather than shared: the staging calls and the scale sit inside it, and the
// assembly of both parents stays what it was.
#pragma once
#include "attn_mla_sparse.hip"   // attn_mla_sparse_combine_kernel<BF16>; attn_mla.hip: MLA_* constants (attn_decode.hip: kv8_16x8<BF16>, mfma16_16<BF16>)

namespace lc {

template <bool BF16>
__global__ __launch_bounds__(256) void attn_mla_sparse_kv8_kernel(const half_t* __restrict__ Qc, const half_t* __restrict__ Qpe,
                                                                  const uint8_t* __restrict__ CKV, const half_t* __restrict__ KPE,
                                                                  half_t* __restrict__ O, float* __restrict__ lse, const int* __restrict__ slots,
                                                                  const float* __restrict__ ckv_scale, float* __restrict__ part_o,
                                                                  float* __restrict__ part_lse, int H, int topk, int num_slots, int S, float sl2,
                                                                  long total_rows) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int i16 = lane & 15, h = lane >> 4;

  // ---- which (token, range, row block): attn_mla_sparse_kernel's logical order
  const int RB = __builtin_amdgcn_readfirstlane((H + 63) / 64);
  const int lid = __builtin_amdgcn_readfirstlane(xcd_remap((int)blockIdx.x, (int)gridDim.x));
  const int ts = __builtin_amdgcn_readfirstlane(lid / RB), rbase = 64 * (lid - ts * RB);   // (rbase < H: RB = ceil(H / 64))
  const int t = __builtin_amdgcn_readfirstlane(ts / S), s_idx = ts - t * S;
  const int Tw = (int)(((unsigned)topk + MLA_KT - 1) / MLA_KT);
  const int t0 = __builtin_amdgcn_readfirstlane((int)((unsigned)(s_idx * Tw) / (unsigned)S));
  const int t1 = __builtin_amdgcn_readfirstlane((int)((unsigned)((s_idx + 1) * Tw) / (unsigned)S));
  const int* __restrict__ srow = slots + (long)t * topk;
  // the latent scale: one scalar load per workgroup
  const float sc = ckv_scale ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, ckv_scale[0]))) : 1.f;

  // ---- this lane's head (heads >= H: head H - 1, nothing stored) and its 18 Q fragments: dims 32 s + 8 h ... of Qc, then of Qpe
  const bool wave_live = rbase + 16 * w < H;   // (wave-uniform)
  const int r = rbase + 16 * w + i16;
  const long grow = (long)t * H + (r < H ? r : H - 1);   // the row of Q, O and lse
  half8_t qf[MLA_KS];
#pragma unroll
  for (int s = 0; s < MLA_DC / 32; ++s) qf[s] = *reinterpret_cast<const half8_t*>(Qc + grow * MLA_DC + 32 * s + 8 * h);
#pragma unroll
  for (int s = 0; s < MLA_DR / 32; ++s) qf[MLA_DC / 32 + s] = *reinterpret_cast<const half8_t*>(Qpe + grow * MLA_DR + 32 * s + 8 * h);

  // ---- the entries of tile u, lane j: slots[t, 64 u + j]; an index behind topk is read inside the row and is -1 (64 u + 63 < topk + 127 < 2^32)
  // Two steps, the load and the select, so that the load's wait sits at the top of the NEXT tile and not behind its issue
  auto fetch_raw = [&](int u) {
    const unsigned j = (unsigned)u * MLA_KT + lane;
    return srow[j < (unsigned)topk ? j : (unsigned)topk - 1];
  };
  auto entries = [&](int u, int raw) { return (unsigned)u * MLA_KT + lane < (unsigned)topk ? raw : -1; };
  auto valid_mask = [&](int sv) { return (unsigned long)__builtin_amdgcn_ballot_w64((unsigned)sv < (unsigned)num_slots); };
  auto wave_bits = [&](unsigned long mask) { return (unsigned)(mask >> (16 * w)) & 0xffffu; };   // (wave-uniform) the mask of this wave's 16 rows

  // ---- tile staging: ten loads a lane, the wave's 16 rows whole.  CKV: load n is rows 16 w + 2 n + (lane >> 5), chunk lane & 31 (two 512-byte
  // rows per instruction, a slot per half-wave); KPE: load n is rows 16 w + 8 n + (lane >> 3), chunk lane & 7.  An invalid entry reads slot 0
  u32x4_t stg[10];
#pragma unroll
  for (int n = 0; n < 10; ++n) stg[n] = u32x4_t{0u, 0u, 0u, 0u};
  const int half = lane >> 5, cchunk = lane & 31;
  auto load_tile = [&](int sv) {
    const int svc = (unsigned)sv < (unsigned)num_slots ? sv : 0;   // clamped once: every address below is inside the pools
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int lo = __builtin_amdgcn_readlane(svc, 16 * w + 2 * n), hi = __builtin_amdgcn_readlane(svc, 16 * w + 2 * n + 1);
      const long row = half ? hi : lo;   // 64-bit: num_slots x 512 may pass 2 GiB
      stg[n] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(CKV) + row * MLA_DC + cchunk * 16);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const long row = __builtin_amdgcn_ds_bpermute(4 * (16 * w + 8 * n + (lane >> 3)), svc);
      stg[8 + n] = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(KPE) + row * (MLA_DR * 2) + (lane & 7) * 16);
    }
  };
  // what goes into the image is a select on the ENTRY's mask bit, never on pool data: bit 2 n + half / 8 n + (lane >> 3) of the wave's 16
  auto keep = [&](unsigned bits, int row, u32x4_t v) { return ((bits >> row) & 1u) ? v : u32x4_t{0u, 0u, 0u, 0u}; };
  auto store_tile = [&](char* img, unsigned long mask) {
    const unsigned cb = wave_bits(mask) >> half, rb = wave_bits(mask) >> (lane >> 3);
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      char* dst = img + (16 * w + 2 * n + half) * MLA_ROW + 32 * cchunk;
      *reinterpret_cast<u32x4_t*>(dst) = keep(cb, 2 * n, kv8_16x8<BF16>(stg[n][0], stg[n][1]));
      *reinterpret_cast<u32x4_t*>(dst + 16) = keep(cb, 2 * n, kv8_16x8<BF16>(stg[n][2], stg[n][3]));
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
      *reinterpret_cast<u32x4_t*>(img + (16 * w + 8 * n + (lane >> 3)) * MLA_ROW + MLA_DC * 2 + (lane & 7) * 16) = keep(rb, 8 * n, stg[8 + n]);
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
  int raw = -1;            // slots[t, ...] of the tile to be staged next, as loaded
  if (t1 > t0) {
    const int sv = entries(t0, fetch_raw(t0));
    raw = fetch_raw(t0 + 1);
    cur = valid_mask(sv);
    if (wave_bits(cur)) load_tile(sv);
    // Q is in its registers from here on, in front of the first tile's stores so that both sets of loads share one round trip (the empty
    // statements: attn_mla_kv8.hip)
#pragma unroll
    for (int s = 0; s < MLA_KS; ++s) asm volatile("" ::"v"(qf[s]));
    store_tile(lds, cur);
  }
#pragma unroll
  for (int s = 0; s < MLA_KS; ++s) asm volatile("" ::"v"(qf[s]));   // (... on the path without a tile too: the waits are decided per path)
  __syncthreads();
  // a wave without a head only moves data and meets the barriers (a loop of its own: attn_mla.hip)
  if (!wave_live) {
    for (int u = t0; u < t1; ++u) {
      char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
      if (u + 1 < t1) {
        const int sv = entries(u + 1, raw);
        raw = fetch_raw(u + 2);
        const unsigned long nm = valid_mask(sv);
        if (wave_bits(nm)) load_tile(sv);
        store_tile(nxt, nm);
      }
      __syncthreads();
    }
    return;
  }
  for (int u = t0; u < t1; ++u) {
    char* img = lds + ((u - t0) & 1) * MLA_TILE;
    const bool more = u + 1 < t1;
    char* nxt = lds + (((u - t0) & 1) ^ 1) * MLA_TILE;
    // the entries of tile u + 1 were fetched at the top of tile u - 1; those of tile u + 2 go out in front of the pool loads
    const int sv = entries(u + 1, raw);
    if (more) raw = fetch_raw(u + 2);
    const unsigned long nm = more ? valid_mask(sv) : 0ul;
    // the whole next tile's loads, in flight under this tile's scores and value product
    if (wave_bits(nm)) load_tile(sv);
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
      // ---- rescale Oᵀ only when some row's maximum moved (the empty statements: attn_mla.hip)
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int db = 0; db < MLA_DB; ++db) {
          asm volatile("" : "+a"(o[db]));
          o[db] *= alpha;
          // back into its AGPRs at once, 16 registers at a time: products left in VGPRs until the value product push the staged registers, whose
          // loads are in flight, out into AGPRs behind a vmcnt(0)
          asm volatile("" : "+a"(o[db]));
          if ((db & 3) == 3) __builtin_amdgcn_sched_barrier(0);
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
    // ---- convert the next tile once and store it under its mask: 64 conversions and 18 LDS writes a lane
    if (more) store_tile(nxt, nm);
    cur = nm;
    __syncthreads();   // the next image is whole; every wave is done reading this one
  }

  // ---- a wave owns its heads: no merge across waves.  The four lane groups of a row hold disjoint keys: sum l once.  The scale comes behind
  // the multiply by 1 / l
  if (r >= H) return;
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
