// tu_attn_decode_paged_kv8.hip — translation unit of the fp8-cache paged decode kernels (attn_decode_paged_kv8.hip:
// attn_decode_paged_kv8_kernel<D, RT>).  launch_attn_decode (tu_attn_decode.hip) decides S and the partials, launches this for a plan with kv8
// set, then the shared combine kernel
#include "attn_decode_paged_kv8.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, int RT>
int launch_kv8_rt(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const long rows = (long)p.B * p.H * p.Nq;
  const int grid = p.B * p.Hkv * S;
  return launch_attn_kernel(attn_decode_paged_kv8_kernel<D, RT>, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, a.Q,
                            reinterpret_cast<const uint8_t*>(a.K), reinterpret_cast<const uint8_t*>(a.V), a.O, a.kv_len, a.block_table, a.k_scale,
                            a.v_scale, part_o, part_lse, p.H, p.Hkv, p.Nq, p.Ncap, p.causal ? 1 : 0, S, attn_scale_log2e(D), rows, p.num_pages,
                            __builtin_ctz((unsigned)p.page_size), p.max_pages);
}

template <int D>
int launch_kv8_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  switch (p.RT) {
    case 1: return launch_kv8_rt<D, 1>(p, S, a, part_o, part_lse);
    case 2: return launch_kv8_rt<D, 2>(p, S, a, part_o, part_lse);
    case 4: return launch_kv8_rt<D, 4>(p, S, a, part_o, part_lse);
    default: return LC_ERR_SHAPE;
  }
}

}  // namespace

int launch_attn_decode_paged_kv8_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.D == 128 ? launch_kv8_d<128>(p, S, a, part_o, part_lse) : launch_kv8_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
