// tu_attn_merge.hip — translation unit of the state-merge kernels (attn_merge.hip: attn_merge_states_kernel<D>, attn_merge_states_bf16_kernel<D>)
// and their launcher: lc_attn_merge_states_f16 / _bf16 (lc_abi.hip) state a MergeCall, check_attn_merge (tu_plan.hip) checks it,
// launch_attn_merge below launches it.  Nothing to plan: one kernel on ceil(T H / (2048 / D)) workgroups, no workspace.
#include "attn_merge.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D>
int launch_merge_d(const MergeCall& c, const MergePtrs& p) {
  constexpr int rows_per_block = 256 / (D / 8);
  const long rows = (long)c.T * c.H;   // (<= 2^31 - 1: check_attn_merge)
  const dim3 grid((unsigned)((rows + rows_per_block - 1) / rows_per_block));
  if (c.bf16)
    return launch_attn_kernel(attn_merge_states_bf16_kernel<D>, grid, dim3(256), 0, p.st, p.Oa, p.lse_a, p.Ob, p.lse_b, p.Oout, p.lse_out, p.cu_q, c.B,
                              c.T, c.H);
  return launch_attn_kernel(attn_merge_states_kernel<D>, grid, dim3(256), 0, p.st, p.Oa, p.lse_a, p.Ob, p.lse_b, p.Oout, p.lse_out, p.cu_q, c.B, c.T,
                            c.H);
}

}  // namespace

int launch_attn_merge(const MergeCall& c, const MergePtrs& p) { return c.D == 128 ? launch_merge_d<128>(c, p) : launch_merge_d<64>(c, p); }

}  // namespace lc
