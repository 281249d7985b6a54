// tu_rope_append_varlen_pos.hip — translation unit of the ragged rotary-embedding + append kernels with per-token rotary positions
// (rope_append_varlen_pos.hip: rope_append_varlen_pos_kernel<D, INTERLEAVED>, _pos_kv8_kernel, _pos_bf16_kernel, _pos_kv8_bf16_kernel): the launcher
// of a checked varlen RopeAppendCall with pos = true, fp16 or bf16 elements (lc_plan.h).  Grid and arguments are tu_rope_append_varlen.hip's, with
// pos_ids behind them
#include "rope_append_varlen_pos.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D, bool INTERLEAVED>
int launch_rope_varlen_pos_d(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const AppendCall& ac = c.a;
  const AppendPtrs& a = p.a;
  const int nblk = (c.T - 1) / kv_append_tokens_per_block(D) + 1;
  const dim3 grid((unsigned)nblk * (unsigned)(ac.Hkv + c.H)), block(256);   // (fits an int: check_rope_append)
  const int lps = __builtin_ctz((unsigned)ac.page_size);
  if (ac.kv_bytes == 1) {
    const auto kern = c.bf16 ? rope_append_varlen_pos_kv8_bf16_kernel<D, INTERLEAVED> : rope_append_varlen_pos_kv8_kernel<D, INTERLEAVED>;
    return launch_attn_kernel(kern, grid, block, 0, a.st, p.Q, a.Knew, a.Vnew, p.Qout, static_cast<uint8_t*>(a.Kpool), static_cast<uint8_t*>(a.Vpool),
                              p.cos_sin, p.cu_q, a.block_table, a.kv_len, a.k_scale, a.v_scale, ac.B, c.H, ac.Hkv, c.T, c.max_nq, ac.num_pages, lps,
                              ac.max_pages, nblk, c.rot_dim, c.max_pos, c.src_row_stride, c.kv_row_stride, p.pos_ids);
  }
  const auto kern = c.bf16 ? rope_append_varlen_pos_bf16_kernel<D, INTERLEAVED> : rope_append_varlen_pos_kernel<D, INTERLEAVED>;
  return launch_attn_kernel(kern, grid, block, 0, a.st, p.Q, a.Knew, a.Vnew, p.Qout, static_cast<half_t*>(a.Kpool), static_cast<half_t*>(a.Vpool),
                            p.cos_sin, p.cu_q, a.block_table, a.kv_len, ac.B, c.H, ac.Hkv, c.T, c.max_nq, ac.num_pages, lps, ac.max_pages, nblk,
                            c.rot_dim, c.max_pos, c.src_row_stride, c.kv_row_stride, p.pos_ids);
}

}  // namespace

int launch_rope_append_varlen_pos(const RopeAppendCall& c, const RopeAppendPtrs& p) {
  const bool il = (c.flags & LC_ROPE_INTERLEAVED) != 0;
  if (c.a.D == 128) return il ? launch_rope_varlen_pos_d<128, true>(c, p) : launch_rope_varlen_pos_d<128, false>(c, p);
  return il ? launch_rope_varlen_pos_d<64, true>(c, p) : launch_rope_varlen_pos_d<64, false>(c, p);
}

}  // namespace lc
