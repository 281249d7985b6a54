// tu_attn_decode_paged_kv8.hip — translation unit of the fp8-cache paged decode kernels (attn_decode_paged_kv8.hip:
// attn_decode_paged_kv8_kernel<D, RT>, byte pools): the range launcher of a DecodeCache::PAGED_KV8 plan.  launch_attn_decode (tu_attn_decode.hip)
// decides S and the partials and runs the shared combine kernel
#include <tuple>

#include "attn_decode_paged_kv8.hip"
#include "lc_plan.h"

#define DECODE_KERNEL attn_decode_paged_kv8_kernel
#define DECODE_CACHE DecodeCache::PAGED_KV8
#define DECODE_KV_T uint8_t
namespace lc {
namespace {
auto decode_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table, a.k_scale, a.v_scale); }
auto decode_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_decode_impl.h"
