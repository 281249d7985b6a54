// tu_attn_chunk.hip — translation unit of the chunked-prefill kernels (attn_chunk.hip: attn_chunk_kernel<D>, attn_chunk_paged_kernel<D>,
// attn_chunk_paged_kv8_kernel<D>): the range launchers of a DecodePlan with RB > 1 row blocks, one per cache kind.  launch_attn_decode
// (tu_attn_decode.hip) decides S and the partials and runs the shared combine kernel; the grid here is B x Hkv x RB x S workgroups.
#include <tuple>

#include "attn_chunk.hip"
#include "lc_plan.h"

namespace lc {
namespace {

// kern: the kernel of (cache kind, D); mid / tail: what it takes between kv_len and part_o, and behind rows (tu_attn_decode_impl.h)
template <int D, typename KV, typename Kern, typename Mid, typename Tail>
int launch_chunk(Kern kern, const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse, const Mid& mid, const Tail& tail) {
  const DecodeCall& c = p.call;
  const long rows = (long)c.B * c.H * c.Nq;
  const int grid = c.B * c.Hkv * p.RB * S;   // (<= 2^31 - 1: check_attn_decode)
  const auto args = std::tuple_cat(std::make_tuple(a.Q, static_cast<const KV*>(a.K), static_cast<const KV*>(a.V), a.O, a.kv_len), mid,
                                   std::make_tuple(part_o, part_lse, c.H, c.Hkv, c.Nq, p.Ncap, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, S, attn_scale_log2e(D), rows),
                                   tail);
  return std::apply([&](auto... x) { return launch_attn_kernel(kern, dim3(grid), dim3(256), DecodeLds<D, 4>::kTotal, a.st, x...); }, args);
}

auto page_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }

}  // namespace

template <>
int launch_attn_chunk_ranges<DecodeCache::FLAT>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const auto none = std::make_tuple();
  return p.call.D == 128 ? launch_chunk<128, half_t>(attn_chunk_kernel<128>, p, S, a, part_o, part_lse, none, none)
                         : launch_chunk<64, half_t>(attn_chunk_kernel<64>, p, S, a, part_o, part_lse, none, none);
}

template <>
int launch_attn_chunk_ranges<DecodeCache::PAGED>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const auto mid = std::make_tuple(a.block_table);
  return p.call.D == 128 ? launch_chunk<128, half_t>(attn_chunk_paged_kernel<128>, p, S, a, part_o, part_lse, mid, page_tail(p.call))
                         : launch_chunk<64, half_t>(attn_chunk_paged_kernel<64>, p, S, a, part_o, part_lse, mid, page_tail(p.call));
}

template <>
int launch_attn_chunk_ranges<DecodeCache::PAGED_KV8>(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  const auto mid = std::make_tuple(a.block_table, a.k_scale, a.v_scale);
  return p.call.D == 128 ? launch_chunk<128, uint8_t>(attn_chunk_paged_kv8_kernel<128>, p, S, a, part_o, part_lse, mid, page_tail(p.call))
                         : launch_chunk<64, uint8_t>(attn_chunk_paged_kv8_kernel<64>, p, S, a, part_o, part_lse, mid, page_tail(p.call));
}

}  // namespace lc
