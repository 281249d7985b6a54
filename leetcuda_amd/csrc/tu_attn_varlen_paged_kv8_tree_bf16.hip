// tu_attn_varlen_paged_kv8_tree_bf16.hip — translation unit of the bfloat16 ragged-batch kernels over the fp8 paged cache with a look-back
// visibility mask per query token (attn_varlen_tree.hip: attn_varlen_paged_kv8_tree_bf16_kernel<D, RT>,
// attn_varlen_chunk_paged_kv8_tree_bf16_kernel<D>): the range launcher of a bf16 varlen DecodePlan with DecodeCall::tree over
// DecodeCache::PAGED_KV8.  The combine kernel is tu_attn_varlen_paged_lse_bf16.hip's
#include <tuple>

#include "attn_varlen_tree.hip"
#include "lc_plan.h"

#define VARLEN_KERNEL attn_varlen_paged_kv8_tree_bf16_kernel
#define VARLEN_CHUNK_KERNEL attn_varlen_chunk_paged_kv8_tree_bf16_kernel
#define VARLEN_CACHE DecodeCache::PAGED_KV8
#define VARLEN_KV_T uint8_t
#define VARLEN_RANGES launch_attn_varlen_tree_bf16_ranges
#define VARLEN_TREE
namespace lc {
namespace {
auto varlen_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table, a.k_scale, a.v_scale); }
auto varlen_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_varlen_impl.h"
