// tu_attn_decode_paged.hip — translation unit of the paged decode kernels (attn_decode_paged.hip: attn_decode_paged_kernel<D, RT>).
// launch_attn_decode (tu_attn_decode.hip) decides S and the partials, launches this for a plan with page_size > 0, then the shared combine kernel
#include "attn_decode_paged.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, int RT>
int launch_paged_rt(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const long rows = (long)p.B * p.H * p.Nq;
  const int grid = p.B * p.Hkv * S;
  return launch_attn_kernel(attn_decode_paged_kernel<D, RT>, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, a.Q, a.K, a.V, a.O, a.kv_len,
                            a.block_table, part_o, part_lse, p.H, p.Hkv, p.Nq, p.Ncap, p.causal ? 1 : 0, S, attn_scale_log2e(D), rows, p.num_pages,
                            __builtin_ctz((unsigned)p.page_size), p.max_pages);
}

template <int D>
int launch_paged_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  switch (p.RT) {
    case 1: return launch_paged_rt<D, 1>(p, S, a, part_o, part_lse);
    case 2: return launch_paged_rt<D, 2>(p, S, a, part_o, part_lse);
    case 4: return launch_paged_rt<D, 4>(p, S, a, part_o, part_lse);
    default: return LC_ERR_SHAPE;
  }
}

}  // namespace

int launch_attn_decode_paged_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.D == 128 ? launch_paged_d<128>(p, S, a, part_o, part_lse) : launch_paged_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
