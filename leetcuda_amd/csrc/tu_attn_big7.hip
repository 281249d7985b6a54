// tu_attn_big7.hip — translation unit of attn_bigd7.hip (D = 256, 64 query rows per wave on v_mfma_f32_16x16x32, fp16 / bf16) — see lc_launch.h
#include "lc_launch.h"
#include "attn_bigd7.hip"

namespace lc {
namespace {
template <bool BF16, bool VT>
int launch_bigd7_t(const AttnPtrs& a, int BH, int N) {
  const int nqb = (N + 255) / 256;   // (N % 256 == 128: the head's last block is half real)
  return launch_attn_kernel(attn_fwd_bigd7_kernel<BF16, VT>, dim3((unsigned)((size_t)nqb * BH)), dim3(256), bd7_lds_bytes(), a.st, a.Q, a.K, a.V, a.O, N, nqb,
                            attn_scale_log2e(256));
}
}  // namespace
// D = 256, N % 256 == 0 (or N % 256 == 128: last block half real), V as [B,H,N,D]; fp16 or bf16
int launch_attn_bigd7(const AttnPtrs& a, int BH, int N, bool bf16) {
  return bf16 ? launch_bigd7_t<true, false>(a, BH, N) : launch_bigd7_t<false, false>(a, BH, N);
}
// the same with V as [B,H,D,N] (fp16: the reference's *_swizzle_qkv entries)
int launch_attn_bigd7_vt(const AttnPtrs& a, int BH, int N) {
  return launch_bigd7_t<false, true>(a, BH, N);
}
}  // namespace lc
