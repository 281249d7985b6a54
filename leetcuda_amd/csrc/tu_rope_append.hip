// tu_rope_append.hip — translation unit of the rotary-embedding + append kernels (rope_append_paged.hip: rope_append_paged_kernel<D, INTERLEAVED>,
// rope_append_paged_kv8_kernel<D, INTERLEAVED>): the launcher of a checked RopeAppendCall (lc_plan.h; check_rope_append in tu_plan.hip decides
// whether there is one)
#include "rope_append_paged.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, bool INTERLEAVED>
int launch_rope_d(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const AppendCall& ac = c.a;
  const AppendPtrs& a = p.a;
  const int bph = (ac.Nq - 1) / kv_append_tokens_per_block(D) + 1;
  const unsigned nkv = (unsigned)(ac.B * ac.Hkv * bph);   // the K/V workgroups come first
  const dim3 grid(nkv + (unsigned)(ac.B * c.H * bph)), block(256);   // (fits an int: check_rope_append)
  const int lps = __builtin_ctz((unsigned)ac.page_size);
  if (ac.kv_bytes == 1)
    return launch_attn_kernel(rope_append_paged_kv8_kernel<D, INTERLEAVED>, grid, block, 0, a.st, p.Q, a.Knew, a.Vnew, p.Qout,
                              static_cast<uint8_t*>(a.Kpool), static_cast<uint8_t*>(a.Vpool), p.cos_sin, a.block_table, a.kv_len, a.k_scale, a.v_scale,
                              c.H, ac.Hkv, ac.Nq, ac.num_pages, lps, ac.max_pages, bph, c.rot_dim, c.max_pos, c.src_row_stride, nkv);
  return launch_attn_kernel(rope_append_paged_kernel<D, INTERLEAVED>, grid, block, 0, a.st, p.Q, a.Knew, a.Vnew, p.Qout, static_cast<half_t*>(a.Kpool),
                            static_cast<half_t*>(a.Vpool), p.cos_sin, a.block_table, a.kv_len, c.H, ac.Hkv, ac.Nq, ac.num_pages, lps, ac.max_pages, bph,
                            c.rot_dim, c.max_pos, c.src_row_stride, nkv);
}

}  // namespace

int launch_rope_append(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const bool il = (c.flags & LC_ROPE_INTERLEAVED) != 0;
  if (c.a.D == 128) return il ? launch_rope_d<128, true>(c, p) : launch_rope_d<128, false>(c, p);
  return il ? launch_rope_d<64, true>(c, p) : launch_rope_d<64, false>(c, p);
}

}  // namespace lc
