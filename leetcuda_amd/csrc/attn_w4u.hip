// attn_w4u.hip — FlashAttention-2 forward, D = 64 / 128, N % 256 == 0 (one block per workgroup: also N % 256 == 128): THE merged-phase 4-wave kernel (round 4: one templated body
// replaces attn_w4g.hip (one block per workgroup), attn_w4p.hip (persistent workgroup), attn_w4n.hip (its D = 128 twin) and the retired
// attn_w4m.hip / attn_w8g.hip; lc_tune_set "attn_nw" = 513 / 515 / 517 select WALK = 0 / 1 / 2).
//
// Same semantics / entry points as attn_fwd.hip (reference: kernels/flash-attn/mma/basic/flash_attn_mma_split_q.cu:55-699,
// dispatcher :769-815; flash_attn_mma_share_qkv.cu:46-769; V handed over as [B,H,D,N]:
// kernels/flash-attn/mma/swizzle/flash_attn_mma_share_qkv_swizzle_qkv.cu:961-1010, flash_attn_mma.py:441-442,716).
//
// template <D, VT, WALK>
//   D     64 or 128 (geometry: attn_mp.h W4G<D>)
//   VT    V is [B,H,D,N]: the tile image in LDS is [D rows][64 kv] (128-B rows, 16-B granule j of row d at slot j ^ ((d >> 1) & 7)),
//         filled by LDS-DMA pieces of 8 d-rows (source stride 2 N bytes), and a Vᵀ fragment is TWO PLAIN ds_read_b64 (kv 4 g .. + 3
//         of kv block 0 / of kv block 1 — the k-slot order the lane-local Pᵀ operand defines) where the [N][D] image needs two
//         ds_read_b64_tr_b16: one for one, same slots, same waits -> the V-transposed entries run at their siblings' speed
//         (round 3: the lock-step kernel, − 27 %).  Conflict-free: tests/test_layouts.py.
//   WALK  0  one 256-row query block per workgroup (grid = #blocks; the hardware dispatches)
//         1  persistent workgroup per CU, static walk w, w + G, w + 2 G, … (round 3's attn_w4p: the K / V / Q streams continue
//            across block seams)
//         2  persistent workgroup per CU, DYNAMIC queue: workgroup on XCD x claims the next id of ITS XCD (x + 8 j) with one
//            atomic per block, one block ahead (issued behind the last P·V MFMAs of block b − 1, broadcast through LDS at block
//            b's prologue barrier: no exposed latency); the counters reset themselves when the last workgroup leaves.
//         3  SPLIT-KV (round 5; grids that do not fill the GPU — the reference author's regime "B <= 4, H <= 48, SeqLen <= 8192",
//            README.md:120): `nsplit` workgroups per 256-row query block, workgroup (block, s) walks the KV tiles
//            [s T / nsplit, (s + 1) T / nsplit) exactly as WALK 0 walks a whole head and writes its NORMALISED partial O (fp16, layout
//            [nsplit][B H][N][D] in the workspace `O` points to) plus the base-2 log-sum-exp of its range per query row
//            (`lse`, [nsplit][B H][N] fp32); attn_split_combine_kernel merges them: O = sum_s 2^(L_s − L) O_s, L = log2 sum_s 2^L_s.
//            (A one-launch form — the last of a query block's nsplit workgroups to arrive merges it, flash-decoding's semaphore — was
//            built and measured in round 5: bit-identical and 2 x slower, one workgroup merging 256 rows is a serial tail of dependent
//            loads against a 4.9 us combine kernel: profiles/r5c_attn_split_fused.log, r5f_small_split_kernel_durations.log; removed.)
// attn_fwd_w4u_causal_kernel<D, VT> (lc_attn_fwd_f16_ex, LC_ATTN_CAUSAL): the same body (attn_w4u_body.inc) with WALK 0 and a causal mask —
// query block b walks tiles 0 .. 4 b + 3, only its diagonal tiles run the masked phase; grid longest block first or head-major.
// The arithmetic of a block is the same instruction for instruction in all three walks and for both V layouts' Q·Kᵀ / softmax
// (VT changes only where Vᵀ fragments come from): WALK 0 / 1 / 2 are bit-identical to each other (GPU test).
//
// What happens BETWEEN two 256-row query blocks of a persistent workgroup: the LDS-DMA of "tile T" and "tile
// T + 1" stages tiles 0 / 1 of the NEXT block into ring slots 0 / 1 — exactly where the next prologue reads them (T % 4 == 0);
// the next block's Q rows are requested right after the last P·V MFMAs and land during the O epilogue; the O staging area sits
// behind ring slots 0 / 1, so the epilogue never touches the slots being filled.  One extra barrier per block.
#pragma once
#include "attn_mp.h"

namespace lc {

// claim counters of the dynamic walk: 1024 rotating slots of 16 words ([0..7] next j per XCD, [8] workgroups that left); zero at
// module load, every launch leaves its slot zeroed again (the last workgroup out resets it).  The host picks the slot (ticket
// mod 1024): launches in flight on different streams use different slots unless 1024 of them are outstanding at once.
constexpr int W4U_QSLOTS = 1024;
static __device__ unsigned int g_w4u_queue[W4U_QSLOTS][16];   // (one array per translation unit that instantiates the kernel)

template <int D>
struct W4U {
  using G = W4G<D>;
  static constexpr int EPI_OFF = 2 * G::SLOT;                                // staging behind ring slots 0, 1
  static constexpr int EPI_BYTES = 4 * 64 * G::EPI_STRIDE;
  static constexpr int MBOX = (EPI_OFF + EPI_BYTES > G::LDS) ? EPI_OFF + EPI_BYTES : G::LDS;   // 16 B: the claimed next block id
  static constexpr int LDS = MBOX + 16;
  static_assert(LDS <= 160 * 1024, "ring + staging must fit a CU's LDS");
};

// W4U_STAMPS (liblc_diag.so only, csrc/diag/attn_w4u_stamps.hip): s_memtime stamps of wave 0 of workgroup 0 at the milestones of a block,
// parked in 256 B of LDS behind the kernel's own allocation and copied to g_w4u_stamps at the end (tools/attn_w4u_stamps.py: where the
// fixed cost of a block goes).  The production library never defines it.
#ifdef W4U_STAMPS
static __device__ unsigned long long g_w4u_stamps[32];
#define W4U_STAMP(k)                                                                                                       \
  do {                                                                                                                     \
    if (blockIdx.x == 0 && wave == 0 && lane == 0)                                                                         \
      *(volatile unsigned long long*)(smem + W4U<D>::LDS + 8 * (k)) = __builtin_readcyclecounter();                         \
  } while (0)
#else
#define W4U_STAMP(k) do { } while (0)
#endif

// The body of both kernels below.  CAUSAL (attn_fwd_w4u_causal_kernel, WALK 0 only): query row i sees keys j <= i.  Query block b
// walks KV tiles 0 .. 4 b + 3 (T per workgroup); tiles 0 .. 4 b − 1 lie wholly below the diagonal and run the non-causal instruction
// stream unchanged, the four diagonal tiles run a separately instantiated phase that replaces masked scores by −inf with a select
// before they are exponentiated, before the overflow guard's row max and (block 0) before the prologue's row max.  `order` 0: grid
// enumerated longest block first (ids v = rank B H + head, rank 0 = the head's last query block), 1: head-major through xcd_remap as
// the non-causal kernel.  Order changes no row's arithmetic.
#define W4U_KVH(bh) (bh)   // K / V head of query head bh: its own (grouped-query forms: attn_w4u_gqa.hip)
template <int D, bool VT, int WALK>
__global__ __launch_bounds__(256) void attn_fwd_w4u_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
    half_t* __restrict__ O, int N, int nqb, float sl2, int nblk, int nwg, int qslot, int nsplit, float* __restrict__ lse) {
  constexpr bool CAUSAL = false;
  constexpr int order = 0;
#include "attn_w4u_body.inc"
}

// causal: one 256-row query block per workgroup, grid = B H N / 256 (nblk), no split-KV, no workspace
template <int D, bool VT>
__global__ __launch_bounds__(256) void attn_fwd_w4u_causal_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ V,
    half_t* __restrict__ O, int N, int nqb, float sl2, int nblk, int order) {
  constexpr bool CAUSAL = true;
  constexpr int WALK = 0;
  const int nwg = nblk, qslot = 0, nsplit = 1;
  float* const lse = nullptr;
#include "attn_w4u_body.inc"
}
#undef W4U_KVH

// ---- split-KV combine: O[row] = sum_s w_s O_s[row] / sum_s w_s, w_s = 2^(L_s[row] - max_s L_s[row]).  One thread per 8 output
// columns (16 B in per split, 16 B out); rows = B H N.  HBM-bound and tiny next to the attention itself: nsplit + 1 rows of D halves.
template <int D>
__global__ __launch_bounds__(256) void attn_split_combine_kernel(const half_t* __restrict__ Op, const float* __restrict__ lse,
                                                                 half_t* __restrict__ O, int nsplit, size_t rows) {
  constexpr int C8 = D / 8;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = idx / C8;
  const int c = (int)(idx % C8);
  if (row >= rows) return;
  float mx = lse[row];
  for (int s = 1; s < nsplit; ++s) mx = fmaxf(mx, lse[(size_t)s * rows + row]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float w = __builtin_amdgcn_exp2f(lse[(size_t)s * rows + row] - mx);
    const half8_t v = *(const half8_t*)(Op + ((size_t)s * rows + row) * D + 8 * c);
    den += w;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += w * (float)v[e];
  }
  const float inv = 1.0f / den;
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)(acc[e] * inv);
  *(half8_t*)(O + row * D + 8 * c) = o;
}

}  // namespace lc
