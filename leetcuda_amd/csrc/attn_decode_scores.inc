// attn_decode_scores.inc — the scores and the online softmax of ONE pipeline step of attn_decode_body.inc, for all RT row tiles: included there,
// inside the step loop, with everything that body declares in scope and a `constexpr bool MASKED` in front of it.  MASKED = false: the loop
// as it always stood in the body.  MASKED = true (the TREE kernels of attn_varlen.hip, on the steps near the workgroup's rows; DESIGN.md
// §4.3o): the row's look-back bit joins the visibility compare.  A text of its own so that a TREE kernel can hold both forms behind one
// wave-uniform branch per step, each a straight run of code in which hipcc runs a row tile's MFMAs under the softmax of the one before (a
// branch per row tile cost the four-row-tile kernels 24 % on every tile; a generic lambda moved the other kernels' schedules).
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      half8_t qf[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s)
        qf[s] = *reinterpret_cast<const half8_t*>(lds + (16 * rt + i16) * L::kQStride + (h * (D / 4) + 8 * s) * 2);
      uint64_t tw = 0;   // MASKED: the row's look-back word, out of the padding of its Q row
      if constexpr (MASKED) tw = *reinterpret_cast<const uint64_t*>(lds + (16 * rt + i16) * L::kQStride + D * 2);
      f32x4_t st[NKB];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma16_16<BF16>(k_frag(kb, s), qf[s], acc);
        st[kb] = acc;
      }
      float mx = DEC_NEG_INF;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          bool vis;   // select on the INDEX: the score may be anything
          if constexpr (LOCAL) vis = (unsigned)(k0 + 16 * kb + r - lim[rt]) + wlo < wlo;
          else vis = k0 + 16 * kb + r < lim[rt];
          // TREE, a step that reaches up to tree_lo: the row's bit d = lim - 1 - j next to the compare; d >= 64 is not governed (a key past the
          // row's limit has d < 0, a huge unsigned: the compare has refused it already)
          if constexpr (MASKED) {
            const unsigned d = (unsigned)(lim[rt] - 1 - (k0 + 16 * kb + r));
            vis = vis && (d > 63u || ((tw >> (d & 63u)) & 1u) != 0);
          }
          const float x = vis ? st[kb][r] * sc2 : DEC_NEG_INF;
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
          pf[rt][kb >> 1][4 * (kb & 1) + r] = cvt16<BF16>(p);
        }
      l[rt] = l[rt] * alpha[rt] + ps;   // (this lane's keys of the step: the four lane groups of a row are summed once, behind the loop)
    }
