// tu_attn_mla_prefill.hip — translation unit of the non-absorbed prefill form of latent attention (attn_mla_prefill.hip:
// attn_mla_prefill_kernel<BF16, RS>) and its launcher: lc_attn_mla_prefill_f16 / _bf16 (lc_abi.hip) state an MlaPrefillCall,
// check_attn_mla_prefill (tu_plan.hip) checks and plans it, launch_attn_mla_prefill below runs the plan: one kernel, no workspace.
#include "attn_mla_prefill.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <bool BF16, int RS>
int launch_mla_prefill(const MlaPrefillPlan& p, const MlaPrefillPtrs& a) {
  const MlaPrefillCall& c = p.call;
  const float sl2 = c.sm_scale * 1.4426950408889634f;
  const dim3 grid((unsigned)((long)p.NB * c.B * c.H));   // (< 2^31: check_attn_mla_prefill)
  return launch_attn_kernel(attn_mla_prefill_kernel<BF16, RS>, grid, dim3(256), MLP_LDS, a.st, a.Q, a.Kn, a.Kpe, a.V, a.O, a.lse, a.cu_q, a.cu_k, c.B,
                            c.H, c.Tq, c.Tk, c.max_nq, c.flags & LC_ATTN_CAUSAL ? 1 : 0, sl2, (long)c.q_row_stride, (long)c.q_head_stride,
                            (long)c.kn_row_stride, (long)c.kn_head_stride, (long)c.kpe_row_stride, (long)c.v_row_stride, (long)c.v_head_stride);
}

}  // namespace

int launch_attn_mla_prefill(const MlaPrefillPlan& p, const MlaPrefillPtrs& a) {
  if (p.call.bf16) return p.RS == 2 ? launch_mla_prefill<true, 2>(p, a) : launch_mla_prefill<true, 1>(p, a);
  return p.RS == 2 ? launch_mla_prefill<false, 2>(p, a) : launch_mla_prefill<false, 1>(p, a);
}

}  // namespace lc
