// tu_mla_index_fp8.hip — translation unit of the fp8 lightning-indexer kernels (mla_index_logits_fp8.hip: mla_index_logits_fp8_kernel<TPW>;
// mla_index_append_fp8.hip: mla_index_append_fp8_kernel<BF16>) and their launchers: lc_mla_index_logits_fp8 and lc_mla_index_append_fp8_f16 /
// _bf16 (lc_abi.hip) state an MlaIndexCall with fp8 set / an MlaIndexAppendCall, check_mla_index_logits / check_mla_index_append_fp8
// (tu_plan.hip) check and plan it.
#include "mla_index_logits_fp8.hip"
#include "mla_index_append_fp8.hip"
#include "lc_plan.h"

namespace lc {
namespace {

int log2_of(int page_size) { return __builtin_ctz((unsigned)page_size); }   // (a power of two: the checks)

template <int TPW>
int launch_logits_fp8(const MlaIndexPlan& p, const MlaIndexPtrs& a) {
  const MlaIndexCall& c = p.call;
  const dim3 grid((unsigned)((long)c.B * p.NB * p.S));   // (< 2^31: check_mla_index_logits bounds B NB 64)
  return launch_attn_kernel(mla_index_logits_fp8_kernel<TPW>, grid, dim3(256), IDX8_LDS, a.st, reinterpret_cast<const uint8_t*>(a.Qi), a.w,
                            reinterpret_cast<const uint8_t*>(a.Ki), a.ks, a.logits, a.cu_q, a.block_table, a.kv_len, c.T, c.max_nq, c.num_pages,
                            log2_of(c.page_size), c.max_pages, (c.flags & LC_ATTN_CAUSAL) ? 1 : 0, p.S, p.NB, (long)c.ld);
}

template <bool BF16>
int launch_append_fp8(const MlaIndexAppendCall& c, const MlaIndexAppendPtrs& a) {
  return launch_attn_kernel(mla_index_append_fp8_kernel<BF16>, dim3((unsigned)((c.T + 3) / 4)), dim3(256), 0, a.st, a.Kinew, a.K8, a.ks, a.cu_q,
                            a.block_table, a.kv_len, c.B, c.T, c.max_nq, c.num_pages, log2_of(c.page_size), c.max_pages, c.row_stride, c.pow2);
}

}  // namespace

// (the plan's token block is four times the tokens a wave owns)
int launch_mla_index_logits_fp8(const MlaIndexPlan& p, const MlaIndexPtrs& a) {
  return p.TB == 16 ? launch_logits_fp8<4>(p, a) : launch_logits_fp8<2>(p, a);
}

int launch_mla_index_append_fp8(const MlaIndexAppendCall& c, const MlaIndexAppendPtrs& a) {
  return c.bf16 ? launch_append_fp8<true>(c, a) : launch_append_fp8<false>(c, a);
}

}  // namespace lc
