// tu_attn_decode.hip — translation unit of the contiguous decode kernels (attn_decode.hip: attn_decode_kernel<D, RT>, attn_decode_combine_kernel<D>)
// and THE launcher of every DecodePlan (lc_plan.h): the three decode families of lc_abi.hip state a DecodeCall, check_attn_decode (tu_plan.hip)
// checks and plans it, launch_attn_decode below owns S, the partials and the combine kernel and reaches the S range workgroups of the plan's cache
// kind through launch_attn_decode_ranges<kind> — tu_attn_decode_impl.h, instantiated here for DecodeCache::FLAT and in tu_attn_decode_paged.hip /
// tu_attn_decode_paged_kv8.hip for the other two, each next to its own kernels.
#include <tuple>

#include "attn_decode.hip"
#include "lc_plan.h"

#define DECODE_KERNEL attn_decode_kernel
#define DECODE_CACHE DecodeCache::FLAT
#define DECODE_KV_T half_t
namespace lc {
namespace {
auto decode_mid(const DecodePtrs&) { return std::make_tuple(); }
auto decode_tail(const DecodeCall&) { return std::make_tuple(); }
}  // namespace
}  // namespace lc
#include "tu_attn_decode_impl.h"

namespace lc {
namespace {

using DecodeRanges = int (*)(const DecodePlan&, int, const DecodePtrs&, float*, float*);
constexpr DecodeRanges kDecodeRanges[] = {launch_attn_decode_ranges<DecodeCache::FLAT>, launch_attn_decode_ranges<DecodeCache::PAGED>,
                                          launch_attn_decode_ranges<DecodeCache::PAGED_KV8>};   // by DecodeCache
// ... and of a plan with RB > 1 row blocks (tu_attn_chunk.hip)
constexpr DecodeRanges kChunkRanges[] = {launch_attn_chunk_ranges<DecodeCache::FLAT>, launch_attn_chunk_ranges<DecodeCache::PAGED>,
                                         launch_attn_chunk_ranges<DecodeCache::PAGED_KV8>};
// ... and of a local plan, whatever its RB (tu_attn_local*.hip)
constexpr DecodeRanges kLocalRanges[] = {launch_attn_local_ranges<DecodeCache::FLAT>, launch_attn_local_ranges<DecodeCache::PAGED>,
                                         launch_attn_local_ranges<DecodeCache::PAGED_KV8>};
// ... and of a varlen plan (tu_attn_varlen_paged*.hip): a ragged batch only exists on a paged cache
constexpr DecodeRanges kVarlenRanges[] = {nullptr, launch_attn_varlen_ranges<DecodeCache::PAGED>, launch_attn_varlen_ranges<DecodeCache::PAGED_KV8>};
// ... with bf16 elements (tu_attn_varlen_paged*_bf16.hip)
constexpr DecodeRanges kVarlenBf16Ranges[] = {nullptr, launch_attn_varlen_bf16_ranges<DecodeCache::PAGED>,
                                              launch_attn_varlen_bf16_ranges<DecodeCache::PAGED_KV8>};
// ... that also write the log-sum-exp (tu_attn_varlen_paged*_lse*.hip)
constexpr DecodeRanges kVarlenLseRanges[] = {nullptr, launch_attn_varlen_lse_ranges<DecodeCache::PAGED>,
                                             launch_attn_varlen_lse_ranges<DecodeCache::PAGED_KV8>};
constexpr DecodeRanges kVarlenLseBf16Ranges[] = {nullptr, launch_attn_varlen_lse_bf16_ranges<DecodeCache::PAGED>,
                                                 launch_attn_varlen_lse_bf16_ranges<DecodeCache::PAGED_KV8>};
// ... with a look-back visibility mask per query token (tu_attn_varlen_paged*_tree*.hip); tree implies lse: the combine launches are the LSE plan's
constexpr DecodeRanges kVarlenTreeRanges[] = {nullptr, launch_attn_varlen_tree_ranges<DecodeCache::PAGED>,
                                              launch_attn_varlen_tree_ranges<DecodeCache::PAGED_KV8>};
constexpr DecodeRanges kVarlenTreeBf16Ranges[] = {nullptr, launch_attn_varlen_tree_bf16_ranges<DecodeCache::PAGED>,
                                                  launch_attn_varlen_tree_bf16_ranges<DecodeCache::PAGED_KV8>};

template <int D>
int launch_decode_combine(long rows, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  constexpr int rows_per_block = 256 / (D / 4);
  return launch_attn_kernel(attn_decode_combine_kernel<D>, dim3((unsigned)((rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, a.st, part_o,
                            part_lse, a.O, rows, S);
}

}  // namespace

// The plan's launch; S > 1 needs decode_workspace_bytes(p) bytes: the caller's buffer (checked by the entry point), else the stream's cached
// workspace; a stream that is being captured without a caller buffer and a failed lease run S = 1 (lc_plan.h: "a launch differs from its plan")
int launch_attn_decode(const DecodePlan& p, const DecodePtrs& a, void* workspace) {
  int S = p.S;
  WorkspaceLease lease;
  float* part = static_cast<float*>(workspace);
  if (S > 1 && !part) {
    if (!stream_is_capturing(a.st)) {
      lease = stream_workspace(a.st, decode_workspace_bytes(p));
      part = static_cast<float*>(lease.ptr);
    }
    if (!part) S = 1;
  }
  const long rows = (long)decode_rows(p.call);
  float* part_o = S > 1 ? part : nullptr;
  float* part_lse = S > 1 ? part + (size_t)S * rows * p.call.D : nullptr;
  const int rc = (p.call.tree ? (p.call.bf16 ? kVarlenTreeBf16Ranges : kVarlenTreeRanges) : p.call.lse ? (p.call.bf16 ? kVarlenLseBf16Ranges : kVarlenLseRanges) : p.call.bf16 ? kVarlenBf16Ranges : p.call.varlen ? kVarlenRanges : p.local ? kLocalRanges : p.RB > 1 ? kChunkRanges : kDecodeRanges)[(int)p.cache](p, S, a, part_o, part_lse);
  if (rc != LC_OK || S == 1) return rc;
  if (p.call.lse) return p.call.bf16 ? launch_attn_varlen_combine_lse_bf16(p, S, a, part_o, part_lse) : launch_attn_varlen_combine_lse(p, S, a, part_o, part_lse);
  if (p.call.bf16) return launch_attn_varlen_combine_bf16(p, S, a, part_o, part_lse);
  if (p.call.varlen) return launch_attn_varlen_combine(p, S, a, part_o, part_lse);   // (rows past cu_q[B] are nobody's: its own combine kernel)
  return p.call.D == 128 ? launch_decode_combine<128>(rows, S, a, part_o, part_lse) : launch_decode_combine<64>(rows, S, a, part_o, part_lse);
}

}  // namespace lc
