// attn_varlen_combine.inc — the body of the four ragged combine kernels (attn_varlen.hip), included textually: a shared __device__ function moved
// the code of the fp16 kernel (DESIGN.md §4.3m).  The includer is a __global__ kernel template <int D> with the arguments (part_o, part_lse, O,
// cu_q, B, T_rows, H, S) and, LSE, `lse` behind them, and states in front
//   constexpr bool BF16   O is rounded fp32 -> bf16 (RNE) at the store, not to fp16
//   constexpr bool LSE    the row's first thread also stores lse[row] (a kernel without the argument states a null `lse` for the name to resolve)
// It is attn_decode_combine_kernel<D> for a ragged call: the same merge of the S partials, in the same order (same bits), for the rows of the tokens
// clamp(cu_q[0], 0, T) ... clamp(cu_q[B], 0, T) - 1 — the range kernels wrote no partial for a token outside them, and its O row is nobody's.
// (A row between those bounds that no sequence owns — a cu_q that is not monotone, a sequence longer than max_nq — merges whatever the workspace
// holds into its own O row: garbage in, garbage out, in bounds.)
// lse[row] = (mx + log2 ws) ln 2 — part_lse is in the log2 domain, ws = sum_s exp2(part_lse_s - mx) — or -inf for a row whose every range met no key.
  constexpr int TPR = D / 4;   // threads per row
  const long row = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  const int d = (threadIdx.x % TPR) * 4;
  const int beg = cu_q[0], end = cu_q[B];
  const long total_rows = (long)T_rows * H;
  if (row < (long)(beg < 0 ? 0 : (beg > T_rows ? T_rows : beg)) * H) return;
  if (row >= (long)(end < 0 ? 0 : (end > T_rows ? T_rows : end)) * H) return;
  float mx = DEC_NEG_INF;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, part_lse[(long)s * total_rows + row]);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  float ws = 0.f;
  if (mx != DEC_NEG_INF) {
    for (int s = 0; s < S; ++s) {
      const float wgt = __builtin_amdgcn_exp2f(part_lse[(long)s * total_rows + row] - mx);
      if (wgt > 0.f) {
        acc += *reinterpret_cast<const f32x4_t*>(part_o + ((long)s * total_rows + row) * D + d) * wgt;
        ws += wgt;
      }
    }
  }
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  half4_t y = {cvt16<BF16>(acc[0] * inv), cvt16<BF16>(acc[1] * inv), cvt16<BF16>(acc[2] * inv), cvt16<BF16>(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * D + d) = y;
  if constexpr (LSE) {
    if (d == 0) lse[row] = mx == DEC_NEG_INF ? DEC_NEG_INF : (mx + log2f(ws)) * 0.6931471805599453f;
  }
