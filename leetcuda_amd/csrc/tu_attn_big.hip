// tu_attn_big.hip — translation unit of the full-width large-head-dim attention kernel (attn_bigd2.hip) — see lc_launch.h
#include "lc_launch.h"
#include "attn_bigd2.hip"
#include "attn_bigd3.hip"

namespace lc {
namespace {
template <int D, bool BF16, bool BD3>   // attn_bigd2 / attn_bigd3 (experimental: 32-row double-buffered tiles)
int launch_bigd2_t(const AttnPtrs& a, int BH, int N) {
  auto kern = BD3 ? attn_fwd_bigd3_kernel<D, BF16> : attn_fwd_bigd2_kernel<D, BF16>;
  constexpr int lds = BD3 ? bigd3_lds_bytes<D>() : bigd2_lds_bytes<D>();
  const int nqb = N / 128;
  return launch_attn_kernel(kern, dim3((unsigned)((size_t)nqb * BH)), dim3(256), lds, a.st, a.Q, a.K, a.V, a.O, N, nqb, attn_scale_log2e(D));
}
}  // namespace

// D in {256, 512}, N % 128 == 0, V as [B,H,N,D]
int launch_attn_bigd2(const AttnPtrs& a, int BH, int N, int D, bool bf16, bool bigd3) {
  if (bigd3) {
    if (D == 512) return bf16 ? launch_bigd2_t<512, true, true>(a, BH, N) : launch_bigd2_t<512, false, true>(a, BH, N);
    if (D == 256) return bf16 ? launch_bigd2_t<256, true, true>(a, BH, N) : launch_bigd2_t<256, false, true>(a, BH, N);
  }
  if (D == 512) return bf16 ? launch_bigd2_t<512, true, false>(a, BH, N) : launch_bigd2_t<512, false, false>(a, BH, N);
  if (D == 256) return bf16 ? launch_bigd2_t<256, true, false>(a, BH, N) : launch_bigd2_t<256, false, false>(a, BH, N);
  return LC_ERR_HEADDIM;
}
}  // namespace lc
