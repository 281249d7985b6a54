// tu_attn_varlen_paged_lse.hip — translation unit of the fp16 ragged-batch kernels over the fp16 paged cache that also write each row's
// log-sum-exp (attn_varlen_lse.hip: attn_varlen_paged_lse_kernel<D, RT>, attn_varlen_chunk_paged_lse_kernel<D>):
// the range launcher of a varlen DecodePlan with DecodeCall::lse over DecodeCache::PAGED, and attn_varlen_combine_lse_kernel<D>, which serves both cache kinds
#include <tuple>

#include "attn_varlen_lse.hip"
#include "lc_plan.h"

#define VARLEN_KERNEL attn_varlen_paged_lse_kernel
#define VARLEN_CHUNK_KERNEL attn_varlen_chunk_paged_lse_kernel
#define VARLEN_CACHE DecodeCache::PAGED
#define VARLEN_KV_T half_t
#define VARLEN_RANGES launch_attn_varlen_lse_ranges
#define VARLEN_LSE
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
int launch_varlen_combine_lse_d(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  constexpr int rows_per_block = 256 / (D / 4);
  const long rows = (long)p.call.T * p.call.H;
  return launch_attn_kernel(attn_varlen_combine_lse_kernel<D>, dim3((unsigned)((rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, a.st,
                            part_o, part_lse, a.O, a.cu_q, p.call.B, p.call.T, p.call.H, S, a.lse);
}

}  // namespace

int launch_attn_varlen_combine_lse(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  return p.call.D == 128 ? launch_varlen_combine_lse_d<128>(p, S, a, part_o, part_lse) : launch_varlen_combine_lse_d<64>(p, S, a, part_o, part_lse);
}

}  // namespace lc
