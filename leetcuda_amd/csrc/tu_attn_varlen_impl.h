// tu_attn_varlen_impl.h — the launchers of the twelve ragged-batch units (tu_attn_varlen_paged*.hip), written once on the model of
// tu_attn_local_impl.h: a varlen plan's kernels take the local kernels' arguments with (cu_q, T) behind them — and `lse` (VarlenOut::LSE) or
// `lse, tree_mask` (VarlenOut::TREE) behind those — the rows of the partials are the T x H global rows, and Nq is the plan's max_nq.
// A unit states its variant and includes this file:
//   VARLEN_CACHE    the DecodeCache it serves (PAGED or PAGED_KV8);  VARLEN_BF16  true / false;  VARLEN_OUT  VarlenOut::PLAIN / LSE / TREE
//   VARLEN_COMBINE  defined (to nothing) by the four units that also hold the combine kernel of their (BF16, LSE): it serves both cache kinds
// and gets launch_attn_varlen_ranges<VARLEN_CACHE, VARLEN_BF16, VARLEN_OUT> (lc_plan.h) — the D / RT dispatch, the grid of B x Hkv x RB x S
// workgroups, the LDS size — on the kernels VarlenKernels (attn_varlen.hip) holds for those flags, and launch_attn_varlen_combine<BF16, LSE>.
#include <tuple>

#include "attn_varlen.hip"
#include "lc_plan.h"

namespace lc {
namespace {

constexpr bool kKv8 = VARLEN_CACHE == DecodeCache::PAGED_KV8, kLse = VARLEN_OUT != VarlenOut::PLAIN, kTree = VARLEN_OUT == VarlenOut::TREE;
using Kernels = VarlenKernels<kKv8, VARLEN_BF16, kLse, kTree>;
using KvT = std::conditional_t<kKv8, uint8_t, half_t>;   // the element type of the kernels' K / V

// what the kernels take between kv_len and part_o, and behind T
auto varlen_mid(const DecodePtrs& a) {
  if constexpr (kKv8) return std::make_tuple(a.block_table, a.k_scale, a.v_scale);
  else return std::make_tuple(a.block_table);
}
auto varlen_out(const DecodePtrs& a) {
  if constexpr (kTree) return std::make_tuple(a.lse, a.tree_mask);
  else if constexpr (kLse) return std::make_tuple(a.lse);
  else return std::make_tuple();
}

template <int D, int RT, typename Kern>
int launch_varlen(Kern kern, const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const DecodeCall& c = p.call;
  const long rows = (long)c.T * c.H;
  const int grid = c.B * c.Hkv * p.RB * S;   // (<= 2^31 - 1: check_attn_decode)
  const auto args = std::tuple_cat(std::make_tuple(a.Q, static_cast<const KvT*>(a.K), static_cast<const KvT*>(a.V), a.O, a.kv_len), varlen_mid(a),
                                   std::make_tuple(part_o, part_lse, c.H, c.Hkv, c.max_nq, p.Ncap, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, S, attn_scale_log2e(D), rows,
                                                   c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages, c.window, a.sinks, a.cu_q, c.T),
                                   varlen_out(a));
  return std::apply([&](auto... x) { return launch_attn_kernel(kern, dim3(grid), dim3(256), DecodeLds<D, RT>::kTotal, a.st, x...); }, args);
}

template <int D>
int launch_varlen_d(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  if (p.RB > 1) return launch_varlen<D, 4>(Kernels::chunk<D>(), p, S, a, part_o, part_lse);
  switch (p.RT) {
    case 1: return launch_varlen<D, 1>(Kernels::ranges<D, 1>(), p, S, a, part_o, part_lse);
    case 2: return launch_varlen<D, 2>(Kernels::ranges<D, 2>(), p, S, a, part_o, part_lse);
    case 4: return launch_varlen<D, 4>(Kernels::ranges<D, 4>(), p, S, a, part_o, part_lse);
    default: return LC_ERR_SHAPE;
  }
}

#ifdef VARLEN_COMBINE
template <int D>
int launch_varlen_combine_d(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  constexpr int rows_per_block = 256 / (D / 4);
  const long rows = (long)p.call.T * p.call.H;
  const dim3 grid((unsigned)((rows + rows_per_block - 1) / rows_per_block));
  const auto kern = VarlenCombine<VARLEN_BF16, kLse>::kernel<D>();
  if constexpr (kLse) return launch_attn_kernel(kern, grid, dim3(256), 0, a.st, part_o, part_lse, a.O, a.cu_q, p.call.B, p.call.T, p.call.H, S, a.lse);
  else return launch_attn_kernel(kern, grid, dim3(256), 0, a.st, part_o, part_lse, a.O, a.cu_q, p.call.B, p.call.T, p.call.H, S);
}
#endif

}  // namespace

template <>
int launch_attn_varlen_ranges<VARLEN_CACHE, VARLEN_BF16, VARLEN_OUT>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.call.D == 128 ? launch_varlen_d<128>(p, S, a, part_o, part_lse) : launch_varlen_d<64>(p, S, a, part_o, part_lse);
}

#ifdef VARLEN_COMBINE
template <>
int launch_attn_varlen_combine<VARLEN_BF16, kLse>(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  return p.call.D == 128 ? launch_varlen_combine_d<128>(p, S, a, part_o, part_lse) : launch_varlen_combine_d<64>(p, S, a, part_o, part_lse);
}
#endif

}  // namespace lc
