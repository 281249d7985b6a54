// tu_attn_varlen_paged.hip — translation unit of the ragged-batch kernels over the fp16 paged cache (attn_varlen.hip: attn_varlen_paged_kernel
// <D, RT>, attn_varlen_chunk_paged_kernel<D>) and of attn_varlen_combine_kernel<D>, which serves both cache kinds: the range launcher of a varlen
// DecodePlan over DecodeCache::PAGED and the combine launch of every varlen plan.  launch_attn_decode (tu_attn_decode.hip) decides S and the partials
#include <tuple>

#include "attn_varlen.hip"
#include "lc_plan.h"

#define VARLEN_KERNEL attn_varlen_paged_kernel
#define VARLEN_CHUNK_KERNEL attn_varlen_chunk_paged_kernel
#define VARLEN_CACHE DecodeCache::PAGED
#define VARLEN_KV_T half_t
namespace lc {
namespace {
auto varlen_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table); }
auto varlen_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_varlen_impl.h"

namespace lc {
namespace {

template <int D>
int launch_varlen_combine_d(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  constexpr int rows_per_block = 256 / (D / 4);
  const long rows = (long)p.call.T * p.call.H;
  return launch_attn_kernel(attn_varlen_combine_kernel<D>, dim3((unsigned)((rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, a.st, part_o,
                            part_lse, a.O, a.cu_q, p.call.B, p.call.T, p.call.H, S);
}

}  // namespace

int launch_attn_varlen_combine(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  return p.call.D == 128 ? launch_varlen_combine_d<128>(p, S, a, part_o, part_lse) : launch_varlen_combine_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
