// tu_attn_decode.hip — translation unit of the decode attention kernels (attn_decode.hip: attn_decode_kernel<D, RT>, attn_decode_combine_kernel<D>)
// and the launcher of a DecodePlan (lc_plan.h).  lc_attn_decode_f16 / lc_attn_decode_paged_f16 (lc_abi.hip) check and plan; this unit launches — see
// lc_launch.h.  A plan with page_size > 0 runs attn_decode_paged_kernel<D, RT> (tu_attn_decode_paged.hip) in place of attn_decode_kernel<D, RT>,
// one with kv8 set attn_decode_paged_kv8_kernel<D, RT> (tu_attn_decode_paged_kv8.hip)
#include "attn_decode.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, int RT>
int launch_decode_rt(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const long rows = (long)p.B * p.H * p.Nq;
  const int grid = p.B * p.Hkv * S;
  return launch_attn_kernel(attn_decode_kernel<D, RT>, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, a.Q, a.K, a.V, a.O, a.kv_len, part_o,
                            part_lse, p.H, p.Hkv, p.Nq, p.Ncap, p.causal ? 1 : 0, S, attn_scale_log2e(D), rows);
}

template <int D>
int launch_decode_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  int rc;
  if (p.kv8) rc = launch_attn_decode_paged_kv8_ranges(p, S, a, part_o, part_lse);   // (tu_attn_decode_paged_kv8.hip)
  else if (p.page_size > 0) rc = launch_attn_decode_paged_ranges(p, S, a, part_o, part_lse);   // (tu_attn_decode_paged.hip; the combine below is shared)
  else
    switch (p.RT) {
      case 1: rc = launch_decode_rt<D, 1>(p, S, a, part_o, part_lse); break;
      case 2: rc = launch_decode_rt<D, 2>(p, S, a, part_o, part_lse); break;
      case 4: rc = launch_decode_rt<D, 4>(p, S, a, part_o, part_lse); break;
      default: return LC_ERR_SHAPE;
    }
  if (rc != LC_OK || S == 1) return rc;
  const long rows = (long)p.B * p.H * p.Nq;
  constexpr int rows_per_block = 256 / (D / 4);
  return launch_attn_kernel(attn_decode_combine_kernel<D>, dim3((unsigned)((rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, a.st,
                            (const float*)part_o, (const float*)part_lse, a.O, rows, S);
}

}  // namespace

// The plan's launch; S > 1 needs decode_workspace_bytes(p) bytes: the caller's buffer (checked by lc_attn_decode_f16), else the stream's cached
// workspace; a stream that is being captured without a caller buffer and a failed lease run S = 1 (lc_plan.h: "a launch differs from its plan")
int launch_attn_decode(const DecodePlan& p, const DecodePtrs& a, void* workspace) {
  int S = p.S;
  WorkspaceLease lease;
  float* part = static_cast<float*>(workspace);
  if (S > 1 && !part) {
    if (!stream_is_capturing(a.st)) {
      lease = stream_workspace(a.st, decode_workspace_bytes(p));
      part = static_cast<float*>(lease.ptr);
    }
    if (!part) S = 1;
  }
  const long rows = (long)p.B * p.H * p.Nq;
  float* part_o = S > 1 ? part : nullptr;
  float* part_lse = S > 1 ? part + (size_t)S * rows * p.D : nullptr;
  return p.D == 128 ? launch_decode_d<128>(p, S, a, part_o, part_lse) : launch_decode_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
