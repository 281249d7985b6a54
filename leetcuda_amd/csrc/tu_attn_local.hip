// tu_attn_local.hip — translation unit of the contiguous sliding-window / sink kernels (attn_local.hip: attn_local_kernel<D, RT>,
// attn_local_chunk_kernel<D>): the range launcher of a local DecodePlan over DecodeCache::FLAT.  launch_attn_decode (tu_attn_decode.hip) decides
// S and the partials and runs the shared combine kernel
#include <tuple>

#include "attn_local.hip"
#include "lc_plan.h"

#define LOCAL_KERNEL attn_local_kernel
#define LOCAL_CHUNK_KERNEL attn_local_chunk_kernel
#define LOCAL_CACHE DecodeCache::FLAT
#define LOCAL_KV_T half_t
namespace lc {
namespace {
auto local_mid(const DecodePtrs&) { return std::make_tuple(); }
auto local_tail(const DecodeCall&) { return std::make_tuple(); }
}  // namespace
}  // namespace lc
#include "tu_attn_local_impl.h"
