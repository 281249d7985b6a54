// tu_attn_gqa.hip — translation unit of the grouped-query lock-step attention kernels (attn_fwd_gqa.hip) and of the launcher that runs an
// attention plan with AttnPlan::gqa > 1 (lc_attn_fwd_f16_gqa): the plan is plan_attn's answer for the same (B H, N, D, V layout, causal,
// knobs) — nothing is decided by Hkv —, each kernel is the `_gqa` twin of the one the MHA call launches — see lc_launch.h
#include <limits.h>
#include <math.h>

#include "lc_plan.h"
#include "attn_fwd_gqa.hip"

namespace lc {
namespace {
template <int D, int NW, bool VT, bool CAUSAL>
int launch_attn_gqa(const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, int kvg, hipStream_t st) {
  constexpr int lds = attn_lds_bytes<D, VT>();
  const int nqb = N / (NW * 32);
  const dim3 grid((unsigned)((size_t)nqb * B * H)), block(NW * 64);
  const float sl2 = (1.0f / sqrtf((float)D)) * 1.4426950408889634f;
  if constexpr (CAUSAL) {
    auto kern = attn_fwd_causal_gqa_kernel<D, NW, VT>;
    if (int rc = set_dyn_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, st, Q, K, V, O, N, nqb, sl2, kvg);
  } else {
    auto kern = attn_fwd_gqa_kernel<D, NW, VT, 0>;
    if (int rc = set_dyn_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, st, Q, K, V, O, N, nqb, sl2, kvg);
  }
  return check_launch();
}
template <int D, bool VT, bool CAUSAL>
int launch_lockstep_gqa(int nw, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, int kvg, hipStream_t st) {
  if (nw == 8) return launch_attn_gqa<D, 8, VT, CAUSAL>(Q, K, V, O, B, H, N, kvg, st);
  if (nw == 4) return launch_attn_gqa<D, 4, VT, CAUSAL>(Q, K, V, O, B, H, N, kvg, st);
  return launch_attn_gqa<D, 2, VT, CAUSAL>(Q, K, V, O, B, H, N, kvg, st);
}
template <bool VT, bool CAUSAL>
int launch_lockstep_gqa_d(int nw, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, int D, int kvg, hipStream_t st) {
  return D == 32   ? launch_lockstep_gqa<32, VT, CAUSAL>(nw, Q, K, V, O, B, H, N, kvg, st)
         : D == 64 ? launch_lockstep_gqa<64, VT, CAUSAL>(nw, Q, K, V, O, B, H, N, kvg, st)
         : D == 96 ? launch_lockstep_gqa<96, VT, CAUSAL>(nw, Q, K, V, O, B, H, N, kvg, st)
                   : launch_lockstep_gqa<128, VT, CAUSAL>(nw, Q, K, V, O, B, H, N, kvg, st);
}
}  // namespace

// K, V: [B, H / p.gqa, N, D] (V: [B, H / p.gqa, D, N] when vt); D in {32, 64, 96, 128} (lc_attn_fwd_f16_gqa checked it)
int launch_attn_plan_gqa(const AttnPlan& p, const half_t* Q, const half_t* K, const half_t* V, half_t* O, int B, int H, int N, int D, bool vt,
                         hipStream_t st) {
  const int g = p.gqa;
  if (D != 32 && D != 64 && D != 96 && D != 128) return LC_ERR_HEADDIM;
  switch (p.kern) {
    case AKern::W4U:
      if (D == 128) return vt ? launch_attn_w4u_gqa_d128t(Q, K, V, O, B, H, N, p.walk, p.nsplit, g, st) : launch_attn_w4u_gqa_d128(Q, K, V, O, B, H, N, p.walk, p.nsplit, g, st);
      if (D == 64) return vt ? launch_attn_w4u_gqa_d64t(Q, K, V, O, B, H, N, p.walk, p.nsplit, g, st) : launch_attn_w4u_gqa_d64(Q, K, V, O, B, H, N, p.walk, p.nsplit, g, st);
      break;
    case AKern::W4I:
      if (!vt) return launch_attn_w4i_gqa(Q, K, V, O, B, H, N, D, p.sched, g, st);
      break;
    case AKern::LOCKSTEP:
      return vt ? launch_lockstep_gqa_d<true, false>(p.nw, Q, K, V, O, B, H, N, D, g, st) : launch_lockstep_gqa_d<false, false>(p.nw, Q, K, V, O, B, H, N, D, g, st);
    case AKern::W4U_CAUSAL:
      if (D == 128) return vt ? launch_attn_w4u_causal_gqa_d128t(Q, K, V, O, B, H, N, p.order, g, st) : launch_attn_w4u_causal_gqa_d128(Q, K, V, O, B, H, N, p.order, g, st);
      if (D == 64) return vt ? launch_attn_w4u_causal_gqa_d64t(Q, K, V, O, B, H, N, p.order, g, st) : launch_attn_w4u_causal_gqa_d64(Q, K, V, O, B, H, N, p.order, g, st);
      break;
    case AKern::LOCKSTEP_CAUSAL:
      return vt ? launch_lockstep_gqa_d<true, true>(p.nw, Q, K, V, O, B, H, N, D, g, st) : launch_lockstep_gqa_d<false, true>(p.nw, Q, K, V, O, B, H, N, D, g, st);
    default: break;
  }
  return LC_ERR_HEADDIM;   // (no plan for D <= 128 gets here: a missing kernel is an error, never another kernel)
}
}  // namespace lc
