// tu_attn_varlen_paged_tree.hip — translation unit of the fp16 ragged-batch kernels over the fp16 paged cache with a look-back visibility mask
// per query token (attn_varlen_tree.hip: attn_varlen_paged_tree_kernel<D, RT>, attn_varlen_chunk_paged_tree_kernel<D>): the
// range launcher of a varlen DecodePlan with DecodeCall::tree over DecodeCache::PAGED.  The combine kernel is tu_attn_varlen_paged_lse.hip's
#include <tuple>

#include "attn_varlen_tree.hip"
#include "lc_plan.h"

#define VARLEN_KERNEL attn_varlen_paged_tree_kernel
#define VARLEN_CHUNK_KERNEL attn_varlen_chunk_paged_tree_kernel
#define VARLEN_CACHE DecodeCache::PAGED
#define VARLEN_KV_T half_t
#define VARLEN_RANGES launch_attn_varlen_tree_ranges
#define VARLEN_TREE
namespace lc {
namespace {
auto varlen_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table); }
auto varlen_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_varlen_impl.h"
