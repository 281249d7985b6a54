// tu_rope_append_varlen_impl.h — the launcher of the three ragged rotary-embedding + append units (tu_rope_append_varlen*.hip), written once: a
// checked varlen RopeAppendCall (lc_plan.h; check_rope_append in tu_plan.hip decides whether there is one) on the kernel RopeVarlenKernel
// (rope_append_varlen.hip) holds for (its pools' element width, bf16, pos).  A unit includes this file and instantiates
// launch_rope_append_varlen<U> for itself (RopeVarlenUnit, lc_plan.h): F16 and BF16 hold the two pool kinds of one element type, POS those of both.
#include <tuple>

#include "rope_append_varlen.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, bool INTERLEAVED, bool KV8, RopeVarlenUnit U>
int launch_rope_varlen_kv(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  constexpr bool POS = U == RopeVarlenUnit::POS;
  using PoolT = std::conditional_t<KV8, uint8_t, half_t>;
  const AppendCall& ac = c.a;
  const AppendPtrs& a = p.a;
  const int nblk = (c.T - 1) / kv_append_tokens_per_block(D) + 1;
  const dim3 grid((unsigned)nblk * (unsigned)(ac.Hkv + c.H)), block(256);   // (fits an int: check_rope_append)
  const int lps = __builtin_ctz((unsigned)ac.page_size);
  // (what a kernel takes behind kv_len, fp8 pools only, and behind kv_row_stride, POS only)
  const auto scales = [&] { if constexpr (KV8) return std::make_tuple(a.k_scale, a.v_scale); else return std::make_tuple(); }();
  const auto pos = [&] { if constexpr (POS) return std::make_tuple(p.pos_ids); else return std::make_tuple(); }();
  const auto args = std::tuple_cat(std::make_tuple(p.Q, a.Knew, a.Vnew, p.Qout, static_cast<PoolT*>(a.Kpool), static_cast<PoolT*>(a.Vpool), p.cos_sin, p.cu_q,
                                                   a.block_table, a.kv_len),
                                   scales, std::make_tuple(ac.B, c.H, ac.Hkv, c.T, c.max_nq, ac.num_pages, lps, ac.max_pages, nblk, c.rot_dim, c.max_pos,
                                                           c.src_row_stride, c.kv_row_stride),
                                   pos);
  const auto run = [&](auto kern) { return std::apply([&](auto... x) { return launch_attn_kernel(kern, grid, block, 0, a.st, x...); }, args); };
  if constexpr (POS)
    return c.bf16 ? run(RopeVarlenKernel<KV8, true, true>::template kernel<D, INTERLEAVED>()) : run(RopeVarlenKernel<KV8, false, true>::template kernel<D, INTERLEAVED>());
  else
    return run(RopeVarlenKernel<KV8, U == RopeVarlenUnit::BF16, false>::template kernel<D, INTERLEAVED>());
}

template <int D, bool INTERLEAVED, RopeVarlenUnit U>
int launch_rope_varlen_d(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  return c.a.kv_bytes == 1 ? launch_rope_varlen_kv<D, INTERLEAVED, true, U>(c, p) : launch_rope_varlen_kv<D, INTERLEAVED, false, U>(c, p);
}

}  // namespace

template <RopeVarlenUnit U>
int launch_rope_append_varlen(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const bool il = (c.flags & LC_ROPE_INTERLEAVED) != 0;
  if (c.a.D == 128) return il ? launch_rope_varlen_d<128, true, U>(c, p) : launch_rope_varlen_d<128, false, U>(c, p);
  return il ? launch_rope_varlen_d<64, true, U>(c, p) : launch_rope_varlen_d<64, false, U>(c, p);
}

}  // namespace lc
