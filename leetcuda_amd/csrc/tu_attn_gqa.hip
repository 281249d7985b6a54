// tu_attn_gqa.hip — translation unit of the grouped-query lock-step attention kernels (attn_fwd_gqa.hip): each is the `_gqa` twin of the kernel
// the MHA call of the same plan launches from tu_core.hip, which also dispatches to this unit (launch_attn_plan) — see lc_launch.h
#define LOCKSTEP_GQA 1
#include "tu_attn_lockstep_impl.h"

namespace lc {
// K, V: [B, H / kvg, N, D] (V: [B, H / kvg, D, N] when vt)
int launch_attn_lockstep_gqa(const AttnPtrs& a, int BH, int N, int D, bool vt, bool causal, int nw, int kvg) {
  return launch_lockstep(a, BH, N, D, vt, causal, nw, kvg);
}
}  // namespace lc
