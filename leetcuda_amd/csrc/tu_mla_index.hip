// tu_mla_index.hip — translation unit of the lightning-indexer kernels (mla_index_logits.hip: mla_index_logits_kernel<BF16>;
// mla_index_topk.hip: mla_index_topk_kernel) and their launchers: lc_mla_index_logits_f16 / _bf16 and lc_mla_index_topk (lc_abi.hip) state an
// MlaIndexCall, check_mla_index_logits / check_mla_index_topk (tu_plan.hip) check and plan it.
#include "mla_index_logits.hip"
#include "mla_index_topk.hip"
#include "lc_plan.h"

namespace lc {
namespace {

int log2_of(int page_size) { return __builtin_ctz((unsigned)page_size); }   // (a power of two: the checks)

template <bool BF16>
int launch_logits(const MlaIndexPlan& p, const MlaIndexPtrs& a) {
  const MlaIndexCall& c = p.call;
  const dim3 grid((unsigned)((long)c.B * p.NB * p.S));   // (< 2^31: check_mla_index_logits bounds B NB 64)
  return launch_attn_kernel(mla_index_logits_kernel<BF16>, grid, dim3(256), IDX_LDS, a.st, a.Qi, a.w, a.Ki, a.logits, a.cu_q, a.block_table,
                            a.kv_len, c.T, c.max_nq, c.num_pages, log2_of(c.page_size), c.max_pages, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, p.S, p.NB,
                            (long)c.ld);
}

}  // namespace

int launch_mla_index_logits(const MlaIndexPlan& p, const MlaIndexPtrs& a) {
  return p.call.bf16 ? launch_logits<true>(p, a) : launch_logits<false>(p, a);
}

// one workgroup per row of slots
int launch_mla_index_topk(const MlaIndexPlan& p, const MlaIndexPtrs& a) {
  const MlaIndexCall& c = p.call;
  return launch_attn_kernel(mla_index_topk_kernel, dim3((unsigned)c.T), dim3(TOPK_THREADS), 0, a.st, (const float*)a.logits, a.slots, a.cu_q,
                            a.block_table, a.kv_len, c.B, c.T, c.max_nq, c.num_pages, log2_of(c.page_size), c.max_pages, (long)c.ld, c.topk,
                            (c.flags & LC_ATTN_CAUSAL) ? 1 : 0);
}

}  // namespace lc
