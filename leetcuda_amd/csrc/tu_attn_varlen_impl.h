// tu_attn_varlen_impl.h — the range launcher of the two ragged-batch units (tu_attn_varlen_paged.hip, tu_attn_varlen_paged_kv8.hip), written
// once on the model of tu_attn_local_impl.h: a varlen plan's kernels take the local kernels' arguments with (cu_q, T) behind them, the rows of
// the partials are the T x H global rows, and Nq is the plan's max_nq.  The includer has included attn_varlen.hip and defines
//   VARLEN_KERNEL   its kernel template <D, RT> (RB = 1);  VARLEN_CHUNK_KERNEL  its kernel template <D> (RB > 1);  VARLEN_CACHE  the DecodeCache
//   it serves;  VARLEN_KV_T  the element type of those kernels' K / V
//   varlen_mid(a), varlen_tail(c)   tuples of what its kernels take between kv_len and part_o, and between rows and window
// and gets launch_attn_varlen_ranges<VARLEN_CACHE> (lc_plan.h): the D / RT dispatch, the grid of B x Hkv x RB x S workgroups, the LDS size.
// The two bf16 units (tu_attn_varlen_paged_bf16.hip, _paged_kv8_bf16.hip) define VARLEN_RANGES launch_attn_varlen_bf16_ranges and get that one
// instead: the same arguments, grid and LDS size on their own kernels.  The four LSE units (tu_attn_varlen_paged*_lse*.hip) define
// VARLEN_RANGES launch_attn_varlen_lse_ranges / _lse_bf16_ranges and VARLEN_LSE: their kernels take `lse` behind T, one more tuple element.
// The four tree units (tu_attn_varlen_paged*_tree*.hip) define VARLEN_RANGES launch_attn_varlen_tree_ranges / _tree_bf16_ranges
// and VARLEN_TREE: their kernels take `lse` and `tree_mask` behind T, two more tuple elements.
#include "lc_plan.h"

#ifndef VARLEN_RANGES
#define VARLEN_RANGES launch_attn_varlen_ranges
#endif
#if defined(VARLEN_TREE)
#define VARLEN_LSE_ARG(a) std::make_tuple((a).lse, (a).tree_mask)
#elif defined(VARLEN_LSE)
#define VARLEN_LSE_ARG(a) std::make_tuple((a).lse)
#else
#define VARLEN_LSE_ARG(a) std::make_tuple()
#endif

namespace lc {
namespace {

template <int D, int RT, typename Kern>
int launch_varlen(Kern kern, const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const DecodeCall& c = p.call;
  const long rows = (long)c.T * c.H;
  const int grid = c.B * c.Hkv * p.RB * S;   // (<= 2^31 - 1: check_attn_decode)
  const auto args = std::tuple_cat(std::make_tuple(a.Q, static_cast<const VARLEN_KV_T*>(a.K), static_cast<const VARLEN_KV_T*>(a.V), a.O, a.kv_len), varlen_mid(a),
                                   std::make_tuple(part_o, part_lse, c.H, c.Hkv, c.max_nq, p.Ncap, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, S, attn_scale_log2e(D), rows),
                                   varlen_tail(c), std::make_tuple(c.window, a.sinks, a.cu_q, c.T), VARLEN_LSE_ARG(a));
  return std::apply([&](auto... x) { return launch_attn_kernel(kern, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, x...); }, args);
}

template <int D>
int launch_varlen_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  if (p.RB > 1) return launch_varlen<D, 4>(VARLEN_CHUNK_KERNEL<D>, p, S, a, part_o, part_lse);
  switch (p.RT) {
    case 1: return launch_varlen<D, 1>(VARLEN_KERNEL<D, 1>, p, S, a, part_o, part_lse);
    case 2: return launch_varlen<D, 2>(VARLEN_KERNEL<D, 2>, p, S, a, part_o, part_lse);
    case 4: return launch_varlen<D, 4>(VARLEN_KERNEL<D, 4>, p, S, a, part_o, part_lse);
    default: return LC_ERR_SHAPE;
  }
}

}  // namespace

template <>
int VARLEN_RANGES<VARLEN_CACHE>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.call.D == 128 ? launch_varlen_d<128>(p, S, a, part_o, part_lse) : launch_varlen_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
