// attn_decode_paged.hip — decode attention over a PAGED KV cache (lc_attn_decode_paged_f16): attn_decode_kernel<D, RT>
// (attn_decode.hip) with one thing replaced — how a logical key row becomes an address.
//   - Kpool / Vpool are [num_pages, Hkv, page_size, D]: one (page, K / V head) is one contiguous run of page_size x D halves; block_table is a
//     device int32[B, max_pages], entry [b][p] = the pool page of logical keys p page_size ... (p + 1) page_size - 1 of batch entry b
//   - page_size is a power of two >= 16, so the 16 keys of a K load group and the 4 / 8 key rows of a V chunk group lie in ONE page: the page, its
//     table entry and its 64-bit base are wave-uniform (scalar loads, SGPR bases), a lane adds the 32-bit offset (key & (page_size - 1)) D 2 + ...
//   - the table entries of step u + 2 are read in iteration u, right behind the loads of step u + 1: no K / V load waits for a table load issued in
//     the same iteration (the prologue reads step 0's entries in front of step 0's loads)
//   - source rows are clamped to L_b - 1 as in the contiguous kernel, which bounds the table index by ceil(L_b / page_size) - 1: entries behind it
//     and pool rows of positions >= L_b are never read.  Page ids are clamped to [0, num_pages - 1] IN THE KERNEL: nothing on the host can check
//     the table, so this clamp is what keeps every address inside the pool
// Partition, softmax, mask, merge and epilogues are the shared body: for the same logical cache the bits are those of attn_decode_kernel<D, RT>.
#pragma once
#include "attn_decode.hip"

namespace lc {

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_decode_paged_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv, int Nq,
                                                                int Ncap, int causal, int S, float sl2, long total_rows, int num_pages, int lps,
                                                                int max_pages) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = false;
  const DecodeLocal lc{};
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
  constexpr bool VARLEN = false;
  constexpr bool BF16 = false;
  const DecodeVarlen vl{};
  constexpr bool LSE = false;
  const DecodeLse ls{};
  constexpr bool TREE = false;
  const DecodeTree tr{};
#include "attn_decode_body.inc"
}

}  // namespace lc
