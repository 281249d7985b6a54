// tu_attn_varlen_paged_kv8_lse.hip — translation unit of the fp16 ragged-batch kernels over the fp8 paged cache that also write each row's
// log-sum-exp (attn_varlen_lse.hip: attn_varlen_paged_kv8_lse_kernel<D, RT>, attn_varlen_chunk_paged_kv8_lse_kernel<D>):
// the range launcher of a varlen DecodePlan with DecodeCall::lse over DecodeCache::PAGED_KV8.  The combine kernel lives in tu_attn_varlen_paged_lse.hip
#include <tuple>

#include "attn_varlen_lse.hip"
#include "lc_plan.h"

#define VARLEN_KERNEL attn_varlen_paged_kv8_lse_kernel
#define VARLEN_CHUNK_KERNEL attn_varlen_chunk_paged_kv8_lse_kernel
#define VARLEN_CACHE DecodeCache::PAGED_KV8
#define VARLEN_KV_T uint8_t
#define VARLEN_RANGES launch_attn_varlen_lse_ranges
#define VARLEN_LSE
namespace lc {
namespace {
auto varlen_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table, a.k_scale, a.v_scale); }
auto varlen_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_varlen_impl.h"
