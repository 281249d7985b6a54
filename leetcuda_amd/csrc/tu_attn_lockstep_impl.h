// tu_attn_lockstep_impl.h — THE launcher of the lock-step attention kernels, causal or not, for the two translation units that hold them:
// tu_core.hip (attn_fwd.hip: attn_fwd_kernel<D, NW, VT, ABL>, attn_fwd_causal_kernel<D, NW, VT>) and, with LOCKSTEP_GQA defined, tu_attn_gqa.hip
// (attn_fwd_gqa.hip: their `_gqa` twins, whose group size kvg = H / Hkv is handed to the kernel; the MHA kernels have no such argument).
#include "lc_launch.h"
#ifdef LOCKSTEP_GQA
#include "attn_fwd_gqa.hip"
#define LOCKSTEP_KERNEL attn_fwd_gqa_kernel
#define LOCKSTEP_CAUSAL_KERNEL attn_fwd_causal_gqa_kernel
#define LOCKSTEP_IS_GQA true
#else
#include "attn_fwd.hip"
#define LOCKSTEP_KERNEL attn_fwd_kernel
#define LOCKSTEP_CAUSAL_KERNEL attn_fwd_causal_kernel
#define LOCKSTEP_IS_GQA false
#endif

namespace lc {
namespace {
template <int D, int NW, bool VT, bool CAUSAL, int ABL = 0>
int launch_lockstep_t(const AttnPtrs& a, int BH, int N, int kvg) {
  const int nqb = N / (NW * 32);
  auto go = [&](auto kern) {
    return launch_attn_kernel_kvg<LOCKSTEP_IS_GQA>(kern, dim3((unsigned)((size_t)nqb * BH)), dim3(NW * 64), attn_lds_bytes<D, VT>(), a.st, kvg, a.Q, a.K, a.V,
                                                   a.O, N, nqb, attn_scale_log2e(D));
  };
  if constexpr (CAUSAL) return go(LOCKSTEP_CAUSAL_KERNEL<D, NW, VT>);
  else return go(LOCKSTEP_KERNEL<D, NW, VT, ABL>);
}
template <int D, bool VT, bool CAUSAL>
int launch_lockstep_nw(int nw, const AttnPtrs& a, int BH, int N, int kvg) {
  if (nw == 8) return launch_lockstep_t<D, 8, VT, CAUSAL>(a, BH, N, kvg);
  if (nw == 4) return launch_lockstep_t<D, 4, VT, CAUSAL>(a, BH, N, kvg);
  return launch_lockstep_t<D, 2, VT, CAUSAL>(a, BH, N, kvg);
}
template <bool VT, bool CAUSAL>
int launch_lockstep_d(int D, int nw, const AttnPtrs& a, int BH, int N, int kvg) {
  return D == 32   ? launch_lockstep_nw<32, VT, CAUSAL>(nw, a, BH, N, kvg)
         : D == 64 ? launch_lockstep_nw<64, VT, CAUSAL>(nw, a, BH, N, kvg)
         : D == 96 ? launch_lockstep_nw<96, VT, CAUSAL>(nw, a, BH, N, kvg)
                   : launch_lockstep_nw<128, VT, CAUSAL>(nw, a, BH, N, kvg);
}
// D in {32, 64, 96, 128} (the caller checked it), nw = 8 / 4 / 2 waves of 32 query rows: N % (32 nw) == 0
int launch_lockstep(const AttnPtrs& a, int BH, int N, int D, bool vt, bool causal, int nw, int kvg) {
  if (causal) return vt ? launch_lockstep_d<true, true>(D, nw, a, BH, N, kvg) : launch_lockstep_d<false, true>(D, nw, a, BH, N, kvg);
  return vt ? launch_lockstep_d<true, false>(D, nw, a, BH, N, kvg) : launch_lockstep_d<false, false>(D, nw, a, BH, N, kvg);
}
}  // namespace
}  // namespace lc
