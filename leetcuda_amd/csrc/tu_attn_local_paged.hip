// tu_attn_local_paged.hip — translation unit of the paged sliding-window / sink kernels (attn_local.hip: attn_local_paged_kernel<D, RT>,
// attn_local_chunk_paged_kernel<D>): the range launcher of a local DecodePlan over DecodeCache::PAGED.  launch_attn_decode (tu_attn_decode.hip)
// decides S and the partials and runs the shared combine kernel
#include <tuple>

#include "attn_local.hip"
#include "lc_plan.h"

#define LOCAL_KERNEL attn_local_paged_kernel
#define LOCAL_CHUNK_KERNEL attn_local_chunk_paged_kernel
#define LOCAL_CACHE DecodeCache::PAGED
#define LOCAL_KV_T half_t
namespace lc {
namespace {
auto local_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table); }
auto local_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_local_impl.h"
