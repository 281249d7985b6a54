// tu_kv_append.hip — translation unit of the append-to-cache kernels (kv_append_paged.hip: kv_append_paged_kernel<D>, kv_append_paged_kv8_kernel<D>):
// the launcher of a checked AppendCall (lc_plan.h; check_kv_append in tu_plan.hip decides whether there is one)
#include "kv_append_paged.hip"
#include "lc_plan.h"

namespace lc {
namespace {

template <int D>
int launch_append_d(const AppendCall& c, const AppendPtrs& a) {
  const int bph = (c.Nq - 1) / kv_append_tokens_per_block(D) + 1;
  const dim3 grid(c.B * c.Hkv * bph), block(256);   // (fits an int: check_kv_append)
  const int lps = __builtin_ctz((unsigned)c.page_size);
  if (c.kv_bytes == 1)
    return launch_attn_kernel(kv_append_paged_kv8_kernel<D>, grid, block, 0, a.st, a.Knew, a.Vnew, static_cast<uint8_t*>(a.Kpool),
                              static_cast<uint8_t*>(a.Vpool), a.block_table, a.kv_len, a.k_scale, a.v_scale, c.Hkv, c.Nq, c.num_pages, lps, c.max_pages,
                              bph);
  return launch_attn_kernel(kv_append_paged_kernel<D>, grid, block, 0, a.st, a.Knew, a.Vnew, static_cast<half_t*>(a.Kpool), static_cast<half_t*>(a.Vpool),
                            a.block_table, a.kv_len, c.Hkv, c.Nq, c.num_pages, lps, c.max_pages, bph);
}

}  // namespace

int launch_kv_append(const AppendCall& c, const AppendPtrs& a) { return c.D == 128 ? launch_append_d<128>(c, a) : launch_append_d<64>(c, a); }

}  // namespace lc
