// attn_w4u_gqa.hip — grouped-query (GQA / MQA) forms of the merged-phase attention kernels of attn_w4u.hip (lc_attn_fwd_f16_gqa):
// Q, O [B,H,N,D], K / V [B,Hkv,N,D] (V also [B,Hkv,D,N]), kvg = H / Hkv, query head bh (flat index into [B H]) reads K / V head
// bh / kvg (flat index into [B Hkv]; H % kvg == 0, so this is head h / kvg of the same batch — the repeat_interleave convention).
//
// SEPARATE kernels under separate names — attn_fwd_w4u_gqa_kernel<D, VT, WALK>, attn_fwd_w4u_causal_gqa_kernel<D, VT> — with the same
// body (attn_w4u_body.inc) and one more argument, used in exactly one place: W4U_KVH, the K / V head of a block's query head, taken once
// per 256-row block (own and next block of a persistent walk).  Every phase statement, wait count and ring slot is attn_w4u.hip's, so a
// GQA call returns the bits the MHA kernel returns on K / V expanded kvg times (GPU test), and an MHA call keeps launching the code
// object it always launched.  Split-KV partials, log-sum-exps and the combine kernel are per QUERY head: unchanged.
#pragma once
#include "attn_w4u.hip"

namespace lc {

#define W4U_KVH(bh) ((size_t)((unsigned)(bh) / (unsigned)kvg))   // (bh < 2^31: the launchers bound the block count by INT_MAX)
template <int D, bool VT, int WALK>
__global__ __launch_bounds__(256) void attn_fwd_w4u_gqa_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
    half_t* __restrict__ O, int N, int nqb, float sl2, int nblk, int nwg, int qslot, int nsplit, float* __restrict__ lse, int kvg) {
  constexpr bool CAUSAL = false;
  constexpr int order = 0;
#include "attn_w4u_body.inc"
}

template <int D, bool VT>
__global__ __launch_bounds__(256) void attn_fwd_w4u_causal_gqa_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
    half_t* __restrict__ O, int N, int nqb, float sl2, int nblk, int order, int kvg) {
  constexpr bool CAUSAL = true;
  constexpr int WALK = 0;
  const int nwg = nblk, qslot = 0, nsplit = 1;
  float* const lse = nullptr;
#include "attn_w4u_body.inc"
}
#undef W4U_KVH

}  // namespace lc
