// tu_mla_append.hip — translation unit of the latent-cache append kernels (mla_append_paged.hip: mla_append_paged_kernel<INTERLEAVED>, _bf16_, _kv8_,
// _kv8_bf16_) and their launcher: lc_mla_append_paged_* (lc_abi.hip) state an MlaAppendCall, check_mla_append (tu_plan.hip) checks it, and
// launch_mla_append below picks the kernel MlaAppendKernel holds for (the latent pool's element width, bf16) and sizes the grid.
#include <tuple>

#include "mla_append_paged.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <bool KV8, bool BF16>
int launch_mla_append_kb(const MlaAppendCall& c, const MlaAppendPtrs& a) {
  using PoolT = std::conditional_t<KV8, uint8_t, half_t>;
  const int tpw = mla_append_tokens_per_wave(c.T);
  const unsigned nlat = (unsigned)((c.T - 1) / (4 * tpw) + 1);
  const unsigned nq = (unsigned)(((long)c.T * c.H - 1) / MLA_APPEND_QROWS + 1);
  const dim3 grid(nlat + nq), block(256);   // (fits an int: check_mla_append)
  const int lps = __builtin_ctz((unsigned)c.page_size);
  // (a kernel of an fp8 pool takes the scale behind the pool)
  const auto scale = [&] { if constexpr (KV8) return std::make_tuple(a.ckv_scale); else return std::make_tuple(); }();
  const auto args = std::tuple_cat(std::make_tuple(a.CKVnew, a.KPEnew, a.Qpe, a.Qpe_out, static_cast<PoolT*>(a.CKVpool)), scale,
                                   std::make_tuple(a.KPEpool, a.gamma, a.cos_sin, a.cu_q, a.block_table, a.kv_len, c.B, c.H, c.T, c.max_nq, c.num_pages,
                                                   lps, c.max_pages, c.max_pos, c.eps, c.ckv_row_stride, c.kpe_row_stride, c.q_row_stride,
                                                   c.q_head_stride, tpw, nlat));
  const auto run = [&](auto kern) { return std::apply([&](auto... x) { return launch_attn_kernel(kern, grid, block, 0, a.st, x...); }, args); };
  return c.flags & LC_ROPE_INTERLEAVED ? run(MlaAppendKernel<KV8, BF16>::template kernel<true>()) : run(MlaAppendKernel<KV8, BF16>::template kernel<false>());
}

}  // namespace

int launch_mla_append(const MlaAppendCall& c, const MlaAppendPtrs& a) {
  if (c.kv8) return c.bf16 ? launch_mla_append_kb<true, true>(c, a) : launch_mla_append_kb<true, false>(c, a);
  return c.bf16 ? launch_mla_append_kb<false, true>(c, a) : launch_mla_append_kb<false, false>(c, a);
}

}  // namespace lc
