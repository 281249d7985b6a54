// tu_attn_big4.hip — translation unit of the D = 1024 pair kernel (attn_bigd4.hip) and of attn_bigd2's V-transposed instantiation
// (D = 256, V as [B,H,D,N]: the reference's *_swizzle_qkv entries reach d = 256) — see lc_launch.h
#include "lc_launch.h"
#include "attn_bigd4.hip"

namespace lc {
// D = 1024, N % 64 == 0, V as [B,H,N,D], fp16
namespace {
template <int SP8>
int launch_bigd4_t(const AttnPtrs& a, int BH, int N) {
  const int nqb = N / 64;
  return launch_attn_kernel(attn_fwd_bigd4_kernel<SP8>, dim3((unsigned)((size_t)nqb * BH)), dim3(256), BD4_LDS, a.st, a.Q, a.K, a.V, a.O, N,
                     (g_tune_attn_bigd_map == 1 ? nqb : -nqb)   /* auto = round-robin over the XCDs: + 3.7 % at twice the fabric bytes (MALL-resident K / V, L2 requests spread), profiles/r5f_bigd_map.log */, attn_scale_log2e(1024),
                     /* KV-walk stagger by XCD: auto = with the round-robin map (+ 1.8 ... 2.1 %, profiles/r5h_bigd_stagger.log; nothing with the contiguous one) */
                     (g_tune_attn_bigd_stagger == 2 || (g_tune_attn_bigd_stagger == 0 && g_tune_attn_bigd_map != 1)) ? 1 : 0);
}
}  // namespace
int launch_attn_bigd4(const AttnPtrs& a, int BH, int N, int span8) {
  // default: a batch's 8 pieces spread over its whole half-phase — with one and a half phases between issue and need
  // (attn_bigd4.hip: half-tile recycling) nothing is gained by issuing early, and the texture-address FIFO likes the pieces apart
  // (profiles/r4i_bigd4_v2.log: 8/8 867, 6/8 862, 4/8 845, 2/8 842 TFLOP/s; the first version of the kernel, with one phase per
  // piece, preferred 2/8: 733 vs 712)
  if (span8 == 2) return launch_bigd4_t<2>(a, BH, N);
  if (span8 == 4) return launch_bigd4_t<4>(a, BH, N);
  if (span8 == 6) return launch_bigd4_t<6>(a, BH, N);
  return launch_bigd4_t<8>(a, BH, N);
}
// D = 256, N % 128 == 0, V as [B,H,D,N], fp16
int launch_attn_bigd2_vt(const AttnPtrs& a, int BH, int N, int D) {
  if (D != 256) return LC_ERR_HEADDIM;
  const int nqb = N / 128;
  return launch_attn_kernel(attn_fwd_bigd2_kernel<256, false, true>, dim3((unsigned)((size_t)nqb * BH)), dim3(256), bigd2_lds_bytes<256>(), a.st, a.Q, a.K, a.V,
                            a.O, N, nqb, attn_scale_log2e(256));
}
}  // namespace lc
