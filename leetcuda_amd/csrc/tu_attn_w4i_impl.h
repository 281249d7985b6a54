// tu_attn_w4i_impl.h — body of the translation units tu_attn_w4i.hip and tu_attn_w4i_gqa.hip: the generated merged-phase attention kernel
// (attn_w4i.hip: one generated hand-ordered asm statement per phase), D in {32, 64, 96, 128}, both schedules.  The includer defines
// LC_AN_SLOWPATH_SYM; with W4I_GQA defined the unit holds the grouped-query forms attn_fwd_w4i_gqa_kernel<D, SCHED> instead, whose group size
// kvg = H / Hkv is handed to the kernel (the MHA unit is only ever handed 1).  The unit exports one record (lc_launch.h AttnW4iUnit).
#include "lc_launch.h"
#include "attn_w4i.hip"
#ifdef W4I_GQA
#define W4I_KERNEL attn_fwd_w4i_gqa_kernel
#define W4I_UNIT g_attn_w4i_gqa
#define W4I_IS_GQA true
#else
#define W4I_KERNEL attn_fwd_w4i_kernel
#define W4I_UNIT g_attn_w4i
#define W4I_IS_GQA false
#endif

namespace lc {
namespace {
template <int D, int SCHED>
int launch_w4i_t(const AttnPtrs& a, int BH, int N, int kvg) {
  const int nqb = N / 256;
  return launch_attn_kernel_kvg<W4I_IS_GQA>(W4I_KERNEL<D, SCHED>, dim3((unsigned)((size_t)nqb * BH)), dim3(256), W4G<D>::LDS, a.st, kvg, a.Q, a.K, a.V, a.O, N,
                                            nqb, attn_scale_log2e(D));
}
int launch_w4i(const AttnPtrs& a, int BH, int N, int D, int sched, int kvg) {
  if (D == 32) return sched ? launch_w4i_t<32, 1>(a, BH, N, kvg) : launch_w4i_t<32, 0>(a, BH, N, kvg);
  if (D == 64) return sched ? launch_w4i_t<64, 1>(a, BH, N, kvg) : launch_w4i_t<64, 0>(a, BH, N, kvg);
  if (D == 96) return sched ? launch_w4i_t<96, 1>(a, BH, N, kvg) : launch_w4i_t<96, 0>(a, BH, N, kvg);
  if (D == 128) return sched ? launch_w4i_t<128, 1>(a, BH, N, kvg) : launch_w4i_t<128, 0>(a, BH, N, kvg);
  return LC_ERR_HEADDIM;
}
int slowpath_w4i(unsigned* out4, int reset) { return attn_slowpath_read(LC_AN_SLOWPATH_SYM, out4, reset); }
}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (a host object: the device pass would emit the constant and ask for device forms of the launchers)
const AttnW4iUnit W4I_UNIT = {launch_w4i, slowpath_w4i};
#endif
}  // namespace lc
