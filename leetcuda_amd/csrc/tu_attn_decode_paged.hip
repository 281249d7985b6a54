// tu_attn_decode_paged.hip — translation unit of the paged decode kernels (attn_decode_paged.hip: attn_decode_paged_kernel<D, RT>): the range
// launcher of a DecodeCache::PAGED plan.  launch_attn_decode (tu_attn_decode.hip) decides S and the partials and runs the shared combine kernel
#include <tuple>

#include "attn_decode_paged.hip"
#include "lc_plan.h"

#define DECODE_KERNEL attn_decode_paged_kernel
#define DECODE_CACHE DecodeCache::PAGED
#define DECODE_KV_T half_t
namespace lc {
namespace {
auto decode_mid(const DecodePtrs& a) { return std::make_tuple(a.block_table); }
auto decode_tail(const DecodeCall& c) { return std::make_tuple(c.num_pages, __builtin_ctz((unsigned)c.page_size), c.max_pages); }
}  // namespace
}  // namespace lc
#include "tu_attn_decode_impl.h"
