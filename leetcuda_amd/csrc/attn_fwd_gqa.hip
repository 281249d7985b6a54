// attn_fwd_gqa.hip — grouped-query (GQA / MQA) forms of the lock-step attention kernels of attn_fwd.hip (lc_attn_fwd_f16_gqa): Q, O
// [B,H,N,D], K / V [B,Hkv,N,D] (V also [B,Hkv,D,N]), kvg = H / Hkv, query head bh reads K / V head bh / kvg.  Separate kernels under
// separate names — attn_fwd_gqa_kernel<D, NW, VT, 0>, attn_fwd_causal_gqa_kernel<D, NW, VT> — with the same body (attn_fwd_body.inc) and
// one more argument that only forms the K / V base of the workgroup's head: the bits of the MHA kernels on K / V expanded kvg times.
#pragma once
#include "attn_fwd.hip"

namespace lc {

#define LC_ATTN_KVH(bh) ((size_t)((unsigned)(bh) / (unsigned)kvg))   // (bh < 2^31: a 1-D grid)
template <int D, int NW, bool VT, int ABL = 0>
__global__ __launch_bounds__(NW * 64, (NW >= 4 ? 2 : 1)) void attn_fwd_gqa_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
    half_t* __restrict__ O, int N, int nqb, float sl2, int kvg) {
  constexpr bool CAUSAL = false;
#include "attn_fwd_body.inc"
}

template <int D, int NW, bool VT>
__global__ __launch_bounds__(NW * 64, (NW >= 4 ? 2 : 1)) void attn_fwd_causal_gqa_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
    half_t* __restrict__ O, int N, int nqb, float sl2, int kvg) {
  constexpr bool CAUSAL = true;
  constexpr int ABL = 0;
#include "attn_fwd_body.inc"
}
#undef LC_ATTN_KVH

}  // namespace lc
