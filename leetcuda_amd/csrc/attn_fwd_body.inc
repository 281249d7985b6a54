// attn_fwd_body.inc — the body of attn_fwd_kernel and attn_fwd_causal_kernel (attn_fwd.hip), included INSIDE each kernel (the
// non-causal kernel keeps its instruction stream: a shared __device__ function changed hipcc's scheduling of it).  The includer defines
// D, NW, VT, ABL and the kernel arguments, plus `constexpr bool CAUSAL` and the macro LC_ATTN_KVH(bh): the K / V head that query head bh
// reads (bh itself in attn_fwd.hip, bh / group size in the grouped-query kernels of attn_fwd_gqa.hip).
  using C = AttnCfg<D>;
  constexpr int NT = NW * 64;
  constexpr int DT = D / 32;   // 32-wide d tiles of Oᵀ
  constexpr int DS = D / 16;   // k-steps of the QKᵀ contraction
  constexpr int VB = VT ? C::VTBYTES : C::VBYTES;
  constexpr int SLOT = C::KBYTES + VB;
  constexpr int K_CHUNKS = KVB * C::CH;
  constexpr int V_CHUNKS = VT ? D * 8 : KVB * C::CH;
  constexpr int KL = (K_CHUNKS + NT - 1) / NT;
  constexpr int VL = (V_CHUNKS + NT - 1) / NT;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_id();
  const int hi = lane >> 5;
  const int l32 = lane & 31;

  // XCD-aware placement: each XCD owns a contiguous range of (b,h) problems, so the nqb workgroups that
  // re-read one head's K/V run on the same XCD (same L2) back to back.
  size_t bh;
  int q0;
  if constexpr (CAUSAL) {
    const int nbh = (int)gridDim.x / nqb, rank = (int)blockIdx.x / nbh;
    bh = (size_t)((int)blockIdx.x - rank * nbh);
    q0 = (nqb - 1 - rank) * (NW * 32) + wave * 32;
  } else {
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    bh = id / nqb;
    q0 = (id - (int)bh * nqb) * (NW * 32) + wave * 32;
  }
  const half_t* Qb = Q + bh * (size_t)N * D;
  const size_t kvh = LC_ATTN_KVH(bh);
  const half_t* Kb = K + kvh * (size_t)N * D;
  const half_t* Vb = V + kvh * (size_t)N * D;
  half_t* Ob = O + bh * (size_t)N * D;

  // ---- Q fragments (B operand of Sᵀ = K·Qᵀ): lane holds Q[q0 + l32][16*s + 8*hi .. +8]
  half8_t qf[DS];
#pragma unroll
  for (int s = 0; s < DS; ++s) {
    qf[s] = *(const half8_t*)(Qb + (size_t)(q0 + l32) * D + 16 * s + 8 * hi);
  }

  // ---- register staging of one K/V tile; per-lane global / LDS offsets are hoisted out of the KV loop
  // (the kernel is instruction-issue bound: no per-tile address arithmetic beyond one 64-bit add per load)
  u32x4_t kst[KL], vst[VL];
  const half_t* kg[KL];
  const half_t* vg[VL];
  int kw[KL], vw[VL];
#pragma unroll
  for (int j = 0; j < KL; ++j) {
    const int idx = tid + j * NT;
    kg[j] = Kb + (size_t)idx * 8;
    kw[j] = (idx / C::CH) * C::KSTRIDE + (idx % C::CH) * 16;
  }
#pragma unroll
  for (int j = 0; j < VL; ++j) {
    const int idx = tid + j * NT;
    if constexpr (!VT) {
      vg[j] = Vb + (size_t)idx * 8;
      vw[j] = C::KBYTES + (idx / C::CH) * C::VSTRIDE + (idx % C::CH) * 16;
    } else {
      vg[j] = Vb + (size_t)(idx >> 3) * N + (idx & 7) * 8;
      vw[j] = C::KBYTES + (idx >> 3) * C::VT_STRIDE + (idx & 7) * 16;
    }
  }
  const size_t kstep = (size_t)KVB * D, vstep = VT ? (size_t)KVB : (size_t)KVB * D;
  auto load_tile = [&](int t) {
#pragma unroll
    for (int j = 0; j < KL; ++j)
      if (K_CHUNKS % NT == 0 || tid + j * NT < K_CHUNKS) kst[j] = *(const u32x4_t*)(kg[j] + t * kstep);
#pragma unroll
    for (int j = 0; j < VL; ++j)
      if (V_CHUNKS % NT == 0 || tid + j * NT < V_CHUNKS) vst[j] = *(const u32x4_t*)(vg[j] + t * vstep);
  };
  auto store_tile = [&](char* slot) {
#pragma unroll
    for (int j = 0; j < KL; ++j)
      if (K_CHUNKS % NT == 0 || tid + j * NT < K_CHUNKS) *(u32x4_t*)(slot + kw[j]) = kst[j];
#pragma unroll
    for (int j = 0; j < VL; ++j)
      if (V_CHUNKS % NT == 0 || tid + j * NT < V_CHUNKS) *(u32x4_t*)(slot + vw[j]) = vst[j];
  };

  // ---- lane-dependent LDS read offsets
  const int k_rd = l32 * C::KSTRIDE + hi * 16;  // + t*32*KSTRIDE + s*32
  int v_rd;                                     // V: + (32t+16u)*VSTRIDE [+8*VSTRIDE] + dt*64
  if constexpr (!VT) {
    const int i = lane & 15, gi = (lane >> 4) & 1;
    v_rd = C::KBYTES + (4 * hi + (i >> 2)) * C::VSTRIDE + (16 * gi + 4 * (i & 3)) * 2;
  } else {
    v_rd = C::KBYTES + l32 * C::VT_STRIDE + (4 * hi) * 2;  // + dt*32*VT_STRIDE + (32t+16u)*2 [+16]
  }

  f32x16_t o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // waves 4..7 are dispatched second and lose every issue arbitration to waves 0..3 (priority, then age):
  // one static s_setprio for the younger half evens the two halves out (measured: the older wave idled
  // 1200 of 4300 cycles per tile at the barrier waiting for its partner)
  if (NW == 8 && wave >= 4) __builtin_amdgcn_s_setprio(1);
  // (CAUSAL: through the tile that holds the block's last row)
  const int T = CAUSAL ? ((q0 - wave * 32) + NW * 32 + KVB - 1) / KVB : N / KVB;
  load_tile(0);
  store_tile(smem);
  // Retire the Q loads HERE: otherwise hipcc carries "qf may still be in flight" into the loop and guards
  // every Q·Kᵀ MFMA with an in-order vmcnt(N) that also drains the K/V prefetch issued a few instructions
  // earlier (the whole HBM latency lands inside the MFMA phase of every tile).
#pragma unroll
  for (int s = 0; s < DS; ++s) asm volatile("" : "+v"(qf[s]));
  __syncthreads();

  // ABL & 32: phase time stamps (s_memtime) of waves 0 and 4 of workgroup 0, tiles 16..19, written as u64
  // over the first bytes of Q (already in registers by then; diagnosis only, clobbers the input!)
  unsigned long long* stamp = reinterpret_cast<unsigned long long*>(const_cast<half_t*>(Q));
  const bool stamping = (ABL & 32) && blockIdx.x == 0 && (wave == 0 || wave == 4) && lane == 0;
  auto STAMP = [&](int t, int k) {
    if constexpr (ABL & 32) {
      if (t >= 16 && t < 20) {
        const unsigned long long c = __builtin_readcyclecounter();
        if (stamping) stamp[((wave >> 2) * 4 + (t - 16)) * 8 + k] = c;
      }
    }
  };
  for (int t = 0; t < T; ++t) {
    char* cur = smem + ((ABL & 8) ? 0 : (t & 1)) * SLOT;
    STAMP(t, 0);
    const bool more = !(ABL & 8) && t + 1 < T;

    // ---- Sᵀ = K·Qᵀ : two 32x32 tiles (kv 0..31, 32..63), 2*DS MFMAs in groups of GQ with the next
    // group's K fragments (ds_read_b128) in flight behind the current group's MFMAs.
    f32x16_t s[2];
    if constexpr (ABL & 4) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[tt][r] = (float)qf[r & (DS - 1)][r & 7] * (float)(t + r);
    } else {
      constexpr int GQ = (DS % 4 == 0) ? 4 : 2;    // fragments per group
      constexpr int NGQ = 2 * DS / GQ;
      half8_t kf[2][GQ];
      auto load_k = [&](int g, half8_t (&dst)[GQ]) {
#pragma unroll
        for (int i = 0; i < GQ; ++i) {
          const int idx = g * GQ + i, tt = idx & 1, ks = idx >> 1;  // two independent accumulator chains
          dst[i] = *(const half8_t*)(cur + k_rd + tt * 32 * C::KSTRIDE + ks * 32);
        }
      };
      load_k(0, kf[0]);
#pragma unroll
      for (int g = 0; g < NGQ; ++g) {
        if (g + 1 < NGQ) load_k(g + 1, kf[(g + 1) & 1]);
#pragma unroll
        for (int i = 0; i < GQ; ++i) {
          const int idx = g * GQ + i, tt = idx & 1, ks = idx >> 1;  // two independent accumulator chains
          s[tt] = mfma32(kf[g & 1][i], qf[ks], ks == 0 ? (f32x16_t)0.f : s[tt]);
        }
        // the K/V global prefetch of tile t+1 is issued behind the first MFMA group: a VMEM issue holds the
        // wave for ~80 cycles, which now overlap MFMAs already queued on the matrix pipe
        __builtin_amdgcn_sched_barrier(0);
        if (g == 0 && more) load_tile(t + 1);
      }
    }
    __builtin_amdgcn_sched_barrier(0);

    STAMP(t, 1);
    if constexpr (CAUSAL) {
      // key 64 t + 32 tt + 8 (r >> 2) + 4 hi + (r & 3) against row q0 + l32 (wave-uniform test: does the tile reach past the wave's first row)
      if (KVB * t + KVB - 1 > q0) {
        const int rel = KVB * t + 4 * hi - (q0 + l32);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (rel + 32 * tt + 8 * (r >> 2) + (r & 3) > 0) s[tt][r] = -INFINITY;
      }
    }
    // ---- online softmax (log2 domain): lane owns query row q = l32, kv columns split with lane^32
    float mt[8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      mt[r] = fmaxf(fmaxf(s[0][r], s[0][r + 8]), fmaxf(s[1][r], s[1][r + 8]));
    float mx = fmaxf(fmaxf(fmaxf(mt[0], mt[1]), fmaxf(mt[2], mt[3])),
                     fmaxf(fmaxf(mt[4], mt[5]), fmaxf(mt[6], mt[7])));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_cand = fmaxf(m_run, mx * sl2);
    // Deferred rescale: while no row's max grows by more than 2^RESCALE_THR keep the old reference max
    // (P is then bounded by 2^RESCALE_THR, exact in fp32 sums and far inside fp16 range) and skip the
    // O / l rescale entirely.  The decision covers ONLY this tile's P, which is exponentiated below, and
    // the previous tile's P·V is already accumulated -> everything at the old scale is scaled exactly once.
    // (CAUSAL: m_cand = −inf only while every key this row has seen is masked: no growth, nothing to rescale)
    const float grow = (CAUSAL && m_cand == -INFINITY) ? 0.f : m_cand - m_run;
    if (!__all(grow <= RESCALE_THR)) {
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_cand);
      m_run = m_cand;
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    }
    STAMP(t, 2);
    // packed fp32 math (v_pk_fma_f32 / v_pk_add_f32): two values per scale-subtract and per row-sum add
    f32x2_t ps2[2] = {f32x2_t{0.f, 0.f}, f32x2_t{0.f, 0.f}};
    const float nm0 = (CAUSAL && m_run == -INFINITY) ? 0.f : -m_run;   // (masked scores are −inf: exp2(−inf + 0) = 0, never −inf + inf)
    const f32x2_t sl2v = {sl2, sl2}, nm = {nm0, nm0};
    half8_t pf[2][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const f32x2_t sv = {s[tt][8 * u + j], s[tt][8 * u + j + 1]};
          const f32x2_t e = __builtin_elementwise_fma(sv, sl2v, nm);
          f32x2_t p;
          p[0] = (ABL & 1) ? e[0] : __builtin_amdgcn_exp2f(e[0]);
          p[1] = (ABL & 1) ? e[1] : __builtin_amdgcn_exp2f(e[1]);
          ps2[(j >> 1) & 1] += p;
          pf[tt][u][j] = (half_t)p[0];
          pf[tt][u][j + 1] = (half_t)p[1];
        }
      }
    }
    {
      const f32x2_t t2 = ps2[0] + ps2[1];
      l_run += t2[0] + t2[1];
    }

    // ---- Oᵀ += Vᵀ·Pᵀ : 4 (tt,u) groups of DT MFMAs on independent accumulators; the next group's Vᵀ
    // fragments (2 transpose reads each) are in flight behind the current group's MFMAs.
    if constexpr (ABL & 2) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int u = 0; u < 2; ++u) asm volatile("" ::"v"(pf[tt][u]));
    } else {
      half8_t vf[2][DT];
      auto load_v = [&](int g, half8_t (&dst)[DT]) {
        const int tt = g >> 1, u = g & 1;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          if constexpr (!VT) {
            const char* p = cur + v_rd + (32 * tt + 16 * u) * C::VSTRIDE + dt * 64;
            dst[dt] = cat4(lds_tr16(p), lds_tr16(p + 8 * C::VSTRIDE));
          } else {
            const char* p = cur + v_rd + dt * 32 * C::VT_STRIDE + (32 * tt + 16 * u) * 2;
            dst[dt] = cat4(*(const half4_t*)p, *(const half4_t*)(p + 16));
          }
        }
      };
      load_v(0, vf[0]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (g < 3) load_v(g + 1, vf[(g + 1) & 1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = mfma32(vf[g & 1][dt], pf[g >> 1][g & 1], o[dt]);
        if (g == 1) {   // LDS writes of tile t+1 ride behind the P·V MFMAs (the other ring slot is idle)
          __builtin_amdgcn_sched_barrier(0);
          if (more) store_tile(smem + ((t & 1) ^ 1) * SLOT);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    STAMP(t, 3);
    if ((ABL & 2) && more) store_tile(smem + ((t & 1) ^ 1) * SLOT);   // (P·V ablated: stage here)
    STAMP(t, 4);
    if (!(ABL & 16)) __syncthreads();
    STAMP(t, 5);
  }

  // ---- epilogue: O = Oᵀ / l ; lane holds row q, 4 consecutive d per register quad
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.0f / l_tot;
  half_t* orow = Ob + (size_t)(q0 + l32) * D;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      half4_t h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = (half_t)(o[dt][4 * rq + j] * inv);
      *(half4_t*)(orow + 32 * dt + 8 * rq + 4 * hi) = h;
    }
  }
