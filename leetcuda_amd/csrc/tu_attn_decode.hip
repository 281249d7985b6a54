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

// ... and of a varlen plan (tu_attn_varlen_paged*.hip; a ragged batch only exists on a paged cache): a ladder from the call's cache kind, bf16, lse
// and tree to the one launcher instantiated for them — what a call states is what it launches
template <DecodeCache C, bool BF16>
int varlen_ranges_out(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  if (p.call.tree) return launch_attn_varlen_ranges<C, BF16, VarlenOut::TREE>(p, S, a, part_o, part_lse);
  if (p.call.lse) return launch_attn_varlen_ranges<C, BF16, VarlenOut::LSE>(p, S, a, part_o, part_lse);
  return launch_attn_varlen_ranges<C, BF16, VarlenOut::PLAIN>(p, S, a, part_o, part_lse);
}
template <DecodeCache C>
int varlen_ranges_bf16(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.call.bf16 ? varlen_ranges_out<C, true>(p, S, a, part_o, part_lse) : varlen_ranges_out<C, false>(p, S, a, part_o, part_lse);
}
int varlen_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse) {
  return p.cache == DecodeCache::PAGED_KV8 ? varlen_ranges_bf16<DecodeCache::PAGED_KV8>(p, S, a, part_o, part_lse)
                                           : varlen_ranges_bf16<DecodeCache::PAGED>(p, S, a, part_o, part_lse);
}
// (rows past cu_q[B] are nobody's: a varlen plan has combine kernels of its own, by bf16 and lse)
template <bool BF16>
int varlen_combine_lse(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  return p.call.lse ? launch_attn_varlen_combine<BF16, true>(p, S, a, part_o, part_lse) : launch_attn_varlen_combine<BF16, false>(p, S, a, part_o, part_lse);
}
int varlen_combine(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse) {
  return p.call.bf16 ? varlen_combine_lse<true>(p, S, a, part_o, part_lse) : varlen_combine_lse<false>(p, S, a, part_o, part_lse);
}

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
  // (bf16, lse and tree are stated by the varlen entries only)
  const int rc = p.call.varlen ? varlen_ranges(p, S, a, part_o, part_lse) : (p.local ? kLocalRanges : p.RB > 1 ? kChunkRanges : kDecodeRanges)[(int)p.cache](p, S, a, part_o, part_lse);
  if (rc != LC_OK || S == 1) return rc;
  if (p.call.varlen) return varlen_combine(p, S, a, part_o, part_lse);
  return p.call.D == 128 ? launch_decode_combine<128>(rows, S, a, part_o, part_lse) : launch_decode_combine<64>(rows, S, a, part_o, part_lse);
}

}  // namespace lc
