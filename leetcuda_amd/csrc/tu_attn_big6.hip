// tu_attn_big6.hip — translation unit of attn_bigd6.hip (D = 512 on v_mfma_f32_16x16x32, fp16 / bf16) — see lc_launch.h
#include "lc_launch.h"
#include "attn_bigd6.hip"

namespace lc {
namespace {
template <bool BF16>
int launch_bigd6_t(const AttnPtrs& a, int BH, int N) {
  const int nqb = N / 128;
  return launch_attn_kernel(attn_fwd_bigd6_kernel<BF16>, dim3((unsigned)((size_t)nqb * BH)), dim3(256), bigd2_lds_bytes<512>(), a.st, a.Q, a.K, a.V, a.O, N,
                            (g_tune_attn_bigd_map == 2 ? -nqb : nqb)   /* auto = XCD-contiguous: round-robin measured - 2 % here, profiles/r5f_bigd_map.log */, attn_scale_log2e(512));
}
}  // namespace
// D = 512, N % 128 == 0, V as [B,H,N,D]; fp16 or bf16
int launch_attn_bigd6(const AttnPtrs& a, int BH, int N, bool bf16) {
  return bf16 ? launch_bigd6_t<true>(a, BH, N) : launch_bigd6_t<false>(a, BH, N);
}
}  // namespace lc
