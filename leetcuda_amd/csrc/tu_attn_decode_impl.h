// tu_attn_decode_impl.h — the range launcher of the three decode units (tu_attn_decode.hip, tu_attn_decode_paged.hip, tu_attn_decode_paged_kv8.hip),
// written once.  The includer has included its kernel source and defines
//   DECODE_KERNEL   its kernel template <D, RT>;  DECODE_CACHE  the DecodeCache it serves;  DECODE_KV_T  the element type of that kernel's K / V
//   decode_mid(a), decode_tail(c)   tuples of what its kernel takes besides the common arguments: between kv_len and part_o, and behind rows
// and gets launch_attn_decode_ranges<DECODE_CACHE> (lc_plan.h): the D / RT dispatch, the grid of B x Hkv x S workgroups, the rows, the LDS size.
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, int RT>
int launch_decode_rt(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const DecodeCall& c = p.call;
  const long rows = (long)c.B * c.H * c.Nq;
  const int grid = c.B * c.Hkv * S;
  const auto args = std::tuple_cat(std::make_tuple(a.Q, static_cast<const DECODE_KV_T*>(a.K), static_cast<const DECODE_KV_T*>(a.V), a.O, a.kv_len), decode_mid(a),
                                   std::make_tuple(part_o, part_lse, c.H, c.Hkv, c.Nq, p.Ncap, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, S, attn_scale_log2e(D), rows),
                                   decode_tail(c));
  return std::apply([&](auto... x) { return launch_attn_kernel(DECODE_KERNEL<D, RT>, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, x...); }, args);
}

template <int D>
int launch_decode_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  switch (p.RT) {
    case 1: return launch_decode_rt<D, 1>(p, S, a, part_o, part_lse);
    case 2: return launch_decode_rt<D, 2>(p, S, a, part_o, part_lse);
    case 4: return launch_decode_rt<D, 4>(p, S, a, part_o, part_lse);
    default: return LC_ERR_SHAPE;
  }
}

}  // namespace

template <>
int launch_attn_decode_ranges<DECODE_CACHE>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.call.D == 128 ? launch_decode_d<128>(p, S, a, part_o, part_lse) : launch_decode_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
