// tu_rope_append_varlen_bf16.hip — translation unit of the bfloat16 ragged rotary-embedding + append kernels (rope_append_varlen_bf16.hip:
// rope_append_varlen_bf16_kernel<D, INTERLEAVED>, rope_append_varlen_kv8_bf16_kernel<D, INTERLEAVED>): the launcher of a checked varlen
// RopeAppendCall with bf16 elements (lc_plan.h).  Grid and arguments are tu_rope_append_varlen.hip's
#include "rope_append_varlen_bf16.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, bool INTERLEAVED>
int launch_rope_varlen_bf16_d(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const AppendCall& ac = c.a;
  const AppendPtrs& a = p.a;
  const int nblk = (c.T - 1) / kv_append_tokens_per_block(D) + 1;
  const dim3 grid((unsigned)nblk * (unsigned)(ac.Hkv + c.H)), block(256);   // (fits an int: check_rope_append)
  const int lps = __builtin_ctz((unsigned)ac.page_size);
  if (ac.kv_bytes == 1)
    return launch_attn_kernel(rope_append_varlen_kv8_bf16_kernel<D, INTERLEAVED>, grid, block, 0, a.st, p.Q, a.Knew, a.Vnew, p.Qout,
                              static_cast<uint8_t*>(a.Kpool), static_cast<uint8_t*>(a.Vpool), p.cos_sin, p.cu_q, a.block_table, a.kv_len, a.k_scale,
                              a.v_scale, ac.B, c.H, ac.Hkv, c.T, c.max_nq, ac.num_pages, lps, ac.max_pages, nblk, c.rot_dim, c.max_pos,
                              c.src_row_stride, c.kv_row_stride);
  return launch_attn_kernel(rope_append_varlen_bf16_kernel<D, INTERLEAVED>, grid, block, 0, a.st, p.Q, a.Knew, a.Vnew, p.Qout,
                            static_cast<half_t*>(a.Kpool), static_cast<half_t*>(a.Vpool), p.cos_sin, p.cu_q, a.block_table, a.kv_len, ac.B, c.H,
                            ac.Hkv, c.T, c.max_nq, ac.num_pages, lps, ac.max_pages, nblk, c.rot_dim, c.max_pos, c.src_row_stride, c.kv_row_stride);
}

}  // namespace

int launch_rope_append_varlen_bf16(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const bool il = (c.flags & LC_ROPE_INTERLEAVED) != 0;
  if (c.a.D == 128) return il ? launch_rope_varlen_bf16_d<128, true>(c, p) : launch_rope_varlen_bf16_d<128, false>(c, p);
  return il ? launch_rope_varlen_bf16_d<64, true>(c, p) : launch_rope_varlen_bf16_d<64, false>(c, p);
}

}  // namespace lc
