// tu_attn_local_impl.h — the range launcher of the three sliding-window / sink units (tu_attn_local.hip, tu_attn_local_paged.hip,
// tu_attn_local_paged_kv8.hip), written once: tu_attn_decode_impl.h and tu_attn_chunk.hip's launcher in one, with the two arguments of a local
// plan (DecodeCall::window, DecodePtrs::sinks) behind everything else.  The includer has included attn_local.hip and defines
//   LOCAL_KERNEL   its kernel template <D, RT> (RB = 1);  LOCAL_CHUNK_KERNEL  its kernel template <D> (RB > 1);  LOCAL_CACHE  the DecodeCache it
//   serves;  LOCAL_KV_T  the element type of those kernels' K / V
//   local_mid(a), local_tail(c)   tuples of what its kernels take between kv_len and part_o, and between rows and window
// and gets launch_attn_local_ranges<LOCAL_CACHE> (lc_plan.h): the D / RT dispatch, the grid of B x Hkv x RB x S workgroups, the rows, the LDS size.
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, int RT, typename Kern>
int launch_local(Kern kern, const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const DecodeCall& c = p.call;
  const long rows = (long)c.B * c.H * c.Nq;
  const int grid = c.B * c.Hkv * p.RB * S;   // (<= 2^31 - 1: check_attn_decode)
  const auto args = std::tuple_cat(std::make_tuple(a.Q, static_cast<const LOCAL_KV_T*>(a.K), static_cast<const LOCAL_KV_T*>(a.V), a.O, a.kv_len), local_mid(a),
                                   std::make_tuple(part_o, part_lse, c.H, c.Hkv, c.Nq, p.Ncap, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, S, attn_scale_log2e(D), rows),
                                   local_tail(c), std::make_tuple(c.window, a.sinks));
  return std::apply([&](auto... x) { return launch_attn_kernel(kern, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, x...); }, args);
}

template <int D>
int launch_local_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  if (p.RB > 1) return launch_local<D, 4>(LOCAL_CHUNK_KERNEL<D>, p, S, a, part_o, part_lse);
  switch (p.RT) {
    case 1: return launch_local<D, 1>(LOCAL_KERNEL<D, 1>, p, S, a, part_o, part_lse);
    case 2: return launch_local<D, 2>(LOCAL_KERNEL<D, 2>, p, S, a, part_o, part_lse);
    case 4: return launch_local<D, 4>(LOCAL_KERNEL<D, 4>, p, S, a, part_o, part_lse);
    default: return LC_ERR_SHAPE;
  }
}

}  // namespace

template <>
int launch_attn_local_ranges<LOCAL_CACHE>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.call.D == 128 ? launch_local_d<128>(p, S, a, part_o, part_lse) : launch_local_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
