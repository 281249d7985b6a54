// tu_attn_mla_sparse_kv8.hip — translation unit of the sparse multi-head latent attention kernel over an fp8 latent pool
// (attn_mla_sparse_kv8.hip: attn_mla_sparse_kv8_kernel<BF16>; attn_mla_sparse_combine_kernel<BF16> of attn_mla_sparse.hip is instantiated here a
// second time) and its launcher: lc_attn_mla_sparse_kv8 / _kv8_bf16 (lc_abi.hip) state an MlaSparseCall with kv8 = true, check_attn_mla_sparse
// (tu_plan.hip) checks and plans it — the plan is the 16-bit call's —, launch_attn_mla_sparse_kv8 below owns S, the partials and the combine
// kernel.
#include "attn_mla_sparse_kv8.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <bool BF16>
int launch_mla_sparse_kv8(const MlaSparsePlan& p, int S, const MlaSparsePtrs& a, float* part_o, float* part_lse) {
  const MlaSparseCall& c = p.call;
  const long rows = (long)c.T * c.H;   // (<= 2^31 - 1: check_attn_mla_sparse)
  const float sl2 = c.sm_scale * 1.4426950408889634f;
  const dim3 grid((unsigned)((long)c.T * p.RB * S));   // (< 2^31: check_attn_mla_sparse bounds T RB 64)
  int rc = launch_attn_kernel(attn_mla_sparse_kv8_kernel<BF16>, grid, dim3(256), MLA_LDS, a.st, a.Qc, a.Qpe, reinterpret_cast<const uint8_t*>(a.CKV),
                              a.KPE, a.O, a.lse, a.slots, a.ckv_scale, part_o, part_lse, c.H, c.topk, c.num_slots, S, sl2, rows);
  if (rc != LC_OK || S == 1) return rc;
  return launch_attn_kernel(attn_mla_sparse_combine_kernel<BF16>, dim3((unsigned)((rows + 1) / 2)), dim3(256), 0, a.st, (const float*)part_o,
                            (const float*)part_lse, a.O, a.lse, rows, S);
}

}  // namespace

// The plan's launch; the workspace rule is launch_attn_mla_sparse's (tu_attn_mla_sparse.hip)
int launch_attn_mla_sparse_kv8(const MlaSparsePlan& p, const MlaSparsePtrs& a, void* workspace) {
  int S = p.S;
  WorkspaceLease lease;
  float* part = static_cast<float*>(workspace);
  if (S > 1 && !part) {
    if (!stream_is_capturing(a.st)) {
      lease = stream_workspace(a.st, mla_sparse_workspace_bytes(p));
      part = static_cast<float*>(lease.ptr);
    }
    if (!part) S = 1;
  }
  const size_t rows = (size_t)p.call.T * p.call.H;
  float* part_o = S > 1 ? part : nullptr;
  float* part_lse = S > 1 ? part + (size_t)S * rows * MLA_DC : nullptr;
  return p.call.bf16 ? launch_mla_sparse_kv8<true>(p, S, a, part_o, part_lse) : launch_mla_sparse_kv8<false>(p, S, a, part_o, part_lse);
}

}  // namespace lc
