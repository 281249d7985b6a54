/*
 * lc_abi.h — C-ABI of libleetcuda_amd.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary for the two hot paths of xlite-dev/LeetCUDA:
 *   kernels/hgemm      (fp16 GEMM,  C[M,N] = A[M,K] · B[K,N])
 *   kernels/flash-attn (FlashAttention-2 forward, O = softmax(QKᵀ/√D)·V)
 *
 * The reference binds these paths as flat lists of free functions
 * `void f(torch::Tensor ...)` registered by two pybind modules:
 *   kernels/hgemm/pybind/hgemm.cc:124-182            (38 exports, module `toy_hgemm` / `hgemm_lib`)
 *   kernels/flash-attn/pybind/flash_attn.cc:168-224  (26 exports + 3 optional, module `flash_attn_lib`)
 * Every one of those names is reachable through `lc_hgemm_call` / `lc_attn_call`
 * (dispatch by the reference's export name) and the typed entry points below.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types; never throws across the boundary
 *   - all data pointers are DEVICE pointers (HBM); outputs are caller-allocated and written in place
 *     (same ownership rule as the reference wrappers, e.g. hgemm_mma_stage.cu:2331-2412)
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, which is what the
 *     reference's `<<<grid, block, smem>>>` launches use)
 *   - return value: LC_OK (0) or a negative lc_status code; launches are asynchronous, launch
 *     failures surface as LC_ERR_LAUNCH, execution faults at the caller's next synchronize
 *     (same as the reference: no sync after launch)
 *   - there is NO CPU fallback anywhere behind this ABI.
 */
#ifndef LC_ABI_H_
#define LC_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LC_ABI_VERSION 2   /* 2: retired round-1 kernel variants, lc_build_info, lc_timer_*, probes moved to lc_diag.h */

typedef enum lc_status {
  LC_OK = 0,
  LC_ERR_ARG = -1,      /* null pointer, unknown enum / entry name                                  */
  LC_ERR_SHAPE = -2,    /* non-positive dims, shape / alignment the requested kernel family cannot tile  */
  LC_ERR_HEADDIM = -3,  /* head dim not supported by this attention family ("headdim not support!")  */
  LC_ERR_LAUNCH = -4,   /* hipLaunchKernel / hipFuncSetAttribute failed                              */
  LC_ERR_VENDOR = -5,   /* hipBLASLt comparator unavailable or failed                                */
  LC_ERR_DEVICE = -6    /* no gfx950 device visible                                                  */
} lc_status;

/* B operand storage.  NN: B is [K,N] row-major.  TN: B is stored [N,K] row-major (== column-major
 * [K,N]); the reference still presents it as a [K,N]-shaped tensor (kernels/hgemm/tools/utils.py:152-156)
 * and takes the layout from the entry-point NAME, never from strides — so does this ABI. */
typedef enum lc_layout { LC_LAYOUT_NN = 0, LC_LAYOUT_TN = 1 } lc_layout;

/* HGEMM kernel families behind the ABI (numeric values are stable; 2, 5, 7, 8, 11 were experiments that
 * measured slower and were retired — passing them returns LC_ERR_ARG). */
typedef enum lc_hgemm_variant {
  LC_HGEMM_AUTO = 0,       /* best available for the shape: the reference's legal shapes (M, N % 128 == 0, K % 32 == 0, K >= 64;
                              hgemm_mma_stage.cu:650,675-676) run MFMA256W4Y when the 256-tileable interior has > 128 tiles (128-wide
                              border strips on MFMA128 in a second launch), MID / MFMA128 otherwise; every other shape RAGGED, KPAD, EDGE or GENERIC */
  LC_HGEMM_MFMA256 = 1,    /* 256x256x64 WG tile, 8 wave64, LDS-DMA double buffer, one barrier / K-tile (simplest)      */
  LC_HGEMM_GENERIC = 3,    /* 64x64x32 edge-predicated MFMA kernel: any M,N,K                                           */
  LC_HGEMM_MFMA256P2 = 4,  /* 8-wave ping-pong, 2 phases of 16 MFMAs per K tile, DMA issued inside the MFMA clusters:
                              the independently scheduled cross-check of the default kernel                            */
  LC_HGEMM_MFMA128 = 6,    /* 128x128x64 tile, 4 wave64: M, N multiples of 128 (the reference's own tile), K of 32 (>= 64)  */
  LC_HGEMM_MFMA256W4B = 9, /* 256x256x64 tile, FOUR wave64 with 128x128 wave tiles, A ring of 2 + B ring of 3 K tiles,      */
                           /* v_mfma_f32_32x32x16_f16, global_load_lds DMA (64-bit addresses: the fallback for > 2 GiB spans) */
  LC_HGEMM_MFMA256W4C = 10, /* W4B with buffer_load ... lds (descriptor + scalar offset) DMA: the 32x32x16 baseline         */
  LC_HGEMM_MFMA256W4X = 12, /* W4C's ring / DMA schedule with v_mfma_f32_16x16x32_f16 (8 x 8 blocks of 16 x 16 per wave):   */
                            /* fewer joules per FLOP at the board power cap (hgemm_w4x.hip, compiler-scheduled; TN only)   */
  LC_HGEMM_MFMA256W4Y = 13, /* W4X with the K loop as one generated, hand-ordered instruction stream (hgemm_w4y.hip; TN and  */
                            /* NN): what LC_HGEMM_AUTO launches for large shapes.  Unlike the other 256-tile kernels (M, N % 256 == 0, */
                            /* K % 64 == 0) it takes M, N % 128 == 0 (>= 256) and K % 32 == 0 (>= 64): border strips + a half K-step  */
  LC_HGEMM_MID = 14,        /* the mid-size kernel (hgemm_mid.hip, round 6): (64 | 128) x (128 | 192) x 64 tile, 4 wave64, 2 - 3 slot LDS */
                            /* ring, hand-ordered asm K loop: LC_HGEMM_AUTO's choice between the eight-wave 128-tile kernel (small     */
                            /* grids) and the 256-tile kernel (> 128 tiles of 256 x 256) — n = 1280 .. 2816 square — with the tile that */
                            /* leaves the least work on the busiest CU.  M, N % 64 == 0 (a tile must divide them), K % 32 == 0 (>= 64)  */
  LC_HGEMM_EDGE = 15,       /* the vectorised edge kernel (hgemm_edge.hip, late round 6): 128 x 128 x 64 tile, any M and N, K % 8 == 0 (NN: */
                            /* N % 8 == 0), 16-byte chunks from clamped addresses: what LC_HGEMM_AUTO runs where neither a tiled kernel    */
                            /* nor LC_HGEMM_RAGGED applies (K % 32 != 0, K < 64); K % 8 != 0 / unaligned pointers stay on LC_HGEMM_GENERIC  */
  LC_HGEMM_RAGGED = 16,     /* ragged M / N with K % 32 == 0 (K >= 64), N % 8 == 0 (LC_HGEMM_AUTO's choice there): more than half a CU's worth of 256 x 256  */
                            /* tiles: the interior they divide on hgemm_w4y_kernel, the L-shaped border on hgemm_mid_edge_kernel (128 x 128 tiles of the     */
                            /* mid-size kernel that reach beyond M / N: clamped sources, predicated stores) in a second launch; else all of it on that kernel */
                            /* (tile: "hgemm_ragged_tile"; split-K with workspace partials as "hgemm_mid_splitk" says, one K range under graph capture)      */
  LC_HGEMM_KPAD = 17,       /* K % 32 != 0 (K % 8 == 0, N % 8 == 0, K >= 256) (LC_HGEMM_AUTO from a quarter of a 128 x 128 block per CU on, "hgemm_kpad"): A and B   */
                            /* copied into the stream's workspace with K zero-padded to a multiple of 32, then LC_HGEMM_AUTO on the padded problem (exactly the */
                            /* same result: zeros add nothing; the padded problem runs its workspace-free form — lc_hgemm_kernel_name reports its default launch, */
                            /* a split-K suffix " xN" there does not apply); hgemm_edge_kernel under graph capture / without workspace                          */
  /* the reference's "CUDA-core" ladder as vector-ALU kernels (hgemm_valu.hip; NN only; v_dot2c_f32_f16, fp32 accumulate);
   * shapes a rung does not tile (and TN) run LC_HGEMM_GENERIC */
  LC_HGEMM_VALU_NAIVE = 20,                  /* one thread per C element, operands from global memory                       */
  LC_HGEMM_VALU_SLICED_K = 21,               /* 32x32x32 LDS tile, one C element per thread                                 */
  LC_HGEMM_VALU_T8X8_X4 = 22,                /* 128x128 tile, 8x8 per thread, BK = 8, 8-byte global loads                   */
  LC_HGEMM_VALU_T8X8_X4_PACK = 23,           /* + vector LDS stores                                                         */
  LC_HGEMM_VALU_T8X8_X4_BCF = 24,            /* + bank-conflict-free LDS layout / thread tile                               */
  LC_HGEMM_VALU_T8X8_X4_PACK_BCF = 25,
  LC_HGEMM_VALU_T8X8_X8_PACK_BCF = 26,       /* 16-byte global loads                                                        */
  LC_HGEMM_VALU_T8X8_X8_PACK_BCF_DBUF = 27,  /* + double-buffered LDS                                                       */
  LC_HGEMM_VALU_T8X8_K16 = 28,               /* BK = 16                                                                     */
  LC_HGEMM_VALU_T8X8_K32 = 29,               /* BK = 32                                                                     */
  LC_HGEMM_VALU_T16X8_K32 = 30               /* 256x128 tile, 16x8 per thread                                               */
} lc_hgemm_variant;

/* FlashAttention-2 forward families: the reference's resource policies (kernels/flash-attn/mma/basic/ .cu files), kept as an enum
 * for signature parity ONLY.  `family`, `acc_f32` and `stages` of lc_attn_fwd_f16 are validated and then SELECT NOTHING: the kernel is
 * chosen from (D, N, V layout, B x H and the device's CU count) alone (lc_attn_kernel_name_bh reports it), every kernel accumulates
 * in fp32, and the LDS ring depth is fixed per kernel.  What a family name still decides is the head-dim limit of its ENTRY
 * (lc_attn_call / lc_attn_entry_info: the reference wrappers' switch(d)). */
typedef enum lc_attn_family {
  LC_ATTN_SPLIT_Q = 0,     /* flash_attn_mma_split_q.cu:55      K,V tiles staged in LDS, Q in regs   */
  LC_ATTN_SHARED_QKV = 1,  /* flash_attn_mma_share_qkv.cu:70    one LDS arena time-shared by K and V */
  LC_ATTN_SHARED_KV = 2,   /* flash_attn_mma_share_kv.cu:70                                          */
  LC_ATTN_TILING_QK = 3,   /* flash_attn_mma_tiling_qk.cu:76    Q,K streamed in d-slices             */
  LC_ATTN_TILING_QKV = 4,  /* flash_attn_mma_tiling_qkv.cu:75   Q,K,V streamed in d-slices (FFPA)    */
  LC_ATTN_SPLIT_KV = 5     /* flash_attn_mma_split_kv.cu:33                                          */
} lc_attn_family;

int lc_abi_version(void);
const char* lc_status_string(int status);
/* 0 when a gfx950 device is current, LC_ERR_DEVICE otherwise. Writes the CU count when non-NULL. */
int lc_device_check(int* num_cus);

/* Build identification: the compile flags of this library as one string (e.g. "gfx950 -O3 LC_DIAG=0"); *is_diag = 1
 * when it was built with LC_DIAG=1 (ablation / stamp instantiations compiled in — bench.py and the tests refuse such a
 * library, its diagnosis knobs can make results WRONG).  Never fails. */
const char* lc_build_info(int* is_diag);

/* Run-time selection knobs for A-B benches (not part of the reference surface; correctness never depends on them):
 *   "attn_nw"      attention kernel for D <= 128: 0 = auto; 513 / 515 / 517 = the merged-phase 4-wave kernel attn_fwd_w4u_kernel<D, VT, WALK>
 *                  (attn_w4u.hip: D = 64 / 128, N % 256 == 0, V as [B,H,N,D] or [B,H,D,N]) with WALK 0 (one 256-row query block per
 *                  workgroup), 1 (persistent workgroup per CU, static walk) or 2 (persistent, dynamic per-XCD block queue) — the three compute
 *                  the same bits; 512 = round 2's name for 513; 514 = the same design with every phase as ONE generated asm statement
 *                  (attn_w4i.hip: D = 32 / 64 / 96 / 128, V as [B,H,N,D]; the only merged-phase kernel for D = 96 / 32, where auto picks it);
 *                  8 / 4 / 2 = lock-step kernel with that many waves (any N % (32 x waves) == 0, every D <= 128).  Auto: 515 up to N = 4096
 *                  (D = 64: up to N = 8192), 513 beyond (D = 64 / 128, N % 256 == 0); 514 for D = 96 / 32; else the lock-step kernel
 *   "attn_walk"    block walk of the merged-phase kernel under "attn_nw" = 0: 0 = auto by N (above), 1 / 2 / 3 = WALK 0 / 1 / 2
 *   "attn_w4i_sched" schedule 0 / 1 (default) of attn_w4i's generated phase statements (tools/gen_attn_w4i.py; same bits, A/B knob)
 *   "attn_d1024"   D = 1024 pair kernel (attn_bigd4.hip): a batch of 8 LDS-DMA pieces is spread over this many eighths of a half-phase: 0 = default (8), 2 / 4 / 6
 *   "w4y_sched"    schedule 0..2 of LC_HGEMM_MFMA256W4Y's generated loop body (tools/gen_hgemm_w4y.py; same bits, A/B knob; default 2: k-step pairs per accumulator block)
 *   "hgemm_persist" 1 (default) = LC_HGEMM_MFMA256W4Y as one persistent workgroup per CU walking the C tiles, when their number is a
 *                  multiple of the CU count and larger (same bits as the one-tile launch, 0: + 0.2 % at the cap, + 0.7 % zero-filled)
 *   "hgemm_stagger" K-loop stagger of LC_HGEMM_MFMA256W4Y (hgemm_w4y.hip): the workgroup starts its K walk at tile ((index & mask)
 *                  * step) mod (K / 64) and wraps, index = cx * XCD + cm * tile row + cn * tile column.  0 = auto (cx = 1, mask 7, step
 *                  K / 64 / 8: the eight XCDs start an eighth of K apart), 1 << 27 = off, else cx | cm << 4 | cn << 8 | step << 12 |
 *                  mask << 20 with mask < 128 (bit 27 together with any other bit is refused).  Only the fp32 accumulation order changes:
 *                  results agree with the unstaggered walk to fp16 rounding
 *                  (the K = 128 fp8 kernel shares the stagger and the persistent walk of "hgemm_persist")
 *   "attn_causal_order" grid order of the causal merged-phase kernel: 0 = auto (longest query block first up to 8 rounds of blocks per CU,
 *                  head-major beyond), 1 = longest block first, 2 = head-major (same bits)
 *   "attn_split"   split-KV of the merged-phase kernel (attn_w4u.hip WALK 3) for grids that do not fill the GPU: 0 = auto (a cost model
 *                  over B x H, N, D and the CU count picks 1 / 2 / 4 / 8 / 16 KV ranges per 256-row query block, tu_plan.hip attn_split_auto),
 *                  1 = off: the merged-phase kernel itself on any grid (also switches off the small-grid substitution below), 2 / 4 / 8 / 16 = that
 *                  factor on any grid (N / 64 divisible by it, >= 2 tiles per range).  Partials live in a
 *                  cached per-stream workspace (a few MiB, never freed); while a stream is being captured the unsplit kernel runs
 *                  Small grids the rule leaves unsplit (<= half a GPU of 256-row blocks, N <= 2048) run the 4-wave lock-step kernel, whose
 *                  128-row workgroups fill twice the CUs (+ 9 ... 12 %)
 *   "attn_decode_split" KV ranges per (batch, K / V head) of lc_attn_decode_f16: 0 = auto (the smallest S that gives every CU a workgroup, at least 4
 *                  tiles of 64 cache positions of Ncap per range, at most 64), 1 .. 64 = exactly that many (ranges may be empty: the small test
 *                  shapes reach the split path that way); the name call reports it as " xS".  The paged, fp8 and chunk entries read the
 *                  same knob (a chunk call counts its row blocks among the workgroups the rule hands out)
 *   "attn_bigd_map" block -> query block map of the D = 1024 / D = 512 kernels: 1 = every XCD owns consecutive query blocks of a head (its 32
 *                  CUs share one pass over the head's K / V: the fewest fabric bytes), 2 = round-robin over the XCDs (every XCD streams every
 *                  head: ~2 x the fabric bytes, but the 8 XCDs walk the same heads out of the Infinity Cache); 0 = auto: 2 for D = 1024
 *                  (+ 3.7 %), 1 for D = 512 (2: - 2 %).  Same bits
 *   "attn_bigd_stagger" D = 1024 kernel: the workgroups of XCD x start their KV walk x eighths of the sequence in and wrap (only the fp32 summation
 *                  order changes): 0 = auto (on with the round-robin block map: + 2 %), 1 = off, 2 = on
 *   "hgemm_splitk" split-K of the 128-tile blocks that serve the border strips (M, N % 256 == 128) / the ragged last wave of
 *                  LC_HGEMM_MFMA256W4Y: 0 = auto (2 CUs' worth of blocks per tile when the launch holds fewer blocks than CUs, every K
 *                  range >= 8 tiles), 1 = off, 2 .. 8 = that factor; fp32 partials in the same workspace + a reduce kernel
 *   "hgemm_128w"   waves of LC_HGEMM_MFMA128: 0 = auto (eight — the two k-steps of every K tile on two groups of four waves, summed through LDS at the
 *                  end — on grids of <= 0.6 blocks per CU: + 11 % at 1024^3 / 1536^3; level at 2048^3, slower for NN beyond), 1 = four, 2 = eight
 *   "hgemm_mid"    LC_HGEMM_AUTO's use of LC_HGEMM_MID: 0 = auto (among the 64 / 128 / 192 x 128 / 192 tiles that divide the
 *                  problem the one with the least ceil(workgroups / CUs) x tile area), 1 = never, 12 / 13 / 22 / 23 / 32 / 33 = that tile (rows / 64,
 *                  columns / 64) whenever it divides the problem (A/B knob; also what an explicit LC_HGEMM_MID then runs)
 *   "hgemm_mid_ns" LDS ring slots of LC_HGEMM_MID: 0 = auto (3 when the grid is one round of <= one workgroup per CU, else 2), 2, 3
 *   "hgemm_mid_splitk"  split-K of LC_HGEMM_MID (64 / 128 x 128 tiles; fp32 partials in the stream's workspace + a reduce launch; none under graph
 *                  capture): 0 = auto (a one-round grid on <= half the CUs with >= 64 K tiles: as many ranges as fill the CUs, >= 32 K tiles each,
 *                  <= 8), 1 = never, 2 .. 8 = that many ranges wherever legal (A/B)
 *   "hgemm_tail"   (2 = as 1, but the quadrants on the 128-tile kernel with a workspace split-K: round 5's form, kept for A/B and for shapes with
 *                  border strips; 3 / 4 = as 1 with remainders up to 0.75 / 1.0 of the CUs: measured 8 ... 18 % slower, A/B only)  1 (default) = when the 256-tile grid's last wave holds at most 128 tiles, the generated-loop kernel computes the
 *                  full waves and 128 x 128 blocks the four quadrants of each remaining tile (round 6: on the mid-size kernel, + 4 ... 6 % at 4352 ... 6400); 0 = one launch
 *   "hgemm_tail_tile"  sub-tiles of that tail on the mid-size kernel: 0 = auto (64 x 128 eighths while 8 x the remaining tiles fit one round of the
 *                  CUs, else 128 x 128 quadrants), 1 = eighths, 2 = quadrants (bit-identical results; A/B knob)
 *   "hgemm_ragged" LC_HGEMM_AUTO on ragged M / N with K % 32 == 0 (K >= 64), N % 8 == 0: 0 = LC_HGEMM_RAGGED (the tiled kernels; 128 x 128 tiles with clamped
 *                  sources and predicated stores on what they do not divide), 1 = never (hgemm_edge_kernel alone; A/B knob)
 *   "hgemm_kpad"   LC_HGEMM_AUTO on K % 32 != 0 (K % 8 == 0, N % 8 == 0): 0 = auto (LC_HGEMM_KPAD once the shape holds a quarter of a 128 x 128 block per CU), 1 = never
 *                  (hgemm_edge_kernel), 2 = wherever legal (A/B knob)
 *   "hgemm_ragged_tile"  tile of a ragged problem that runs entirely on hgemm_mid_edge_kernel: 0 = auto (the smallest of 64 x 128, 128 x 128, 128 x 192 (TN) /
 *                  192 x 128 (NN), 192 x 192 (TN) whose grid fits one round of the CUs, three ring slots; else 128 x 128 with two), 12 / 22 / 23 / 32 / 33 = that
 *                  tile where the layout has it (A/B knob)
 *   "hgemm_ragged_fork"  LC_HGEMM_RAGGED's border launch on a per-device side stream forked from / joined to the caller's stream by events (runs beside
 *                  the interior; never while the caller's stream is being captured): 0 = auto (only beside an unsplit last round of the 256-tile grid that
 *                  leaves >= 3 / 8 of the CUs idle: + 4 %; beside full rounds it costs 2 ... 11 %), 1 = never, 2 = always (same bits)
 *   "hgemm_raster" block -> C tile map of the tiled GEMM kernels: 0 = auto (2 when A + B exceed 272 MiB — the 256 MiB Infinity Cache and a margin,
 *                  else 1), 1 = the reference's block swizzle (N panels of swizzle_stride columns, every XCD a contiguous id
 *                  range), 2 = XCD super-block raster (16 x 16 tile steps shared through the Infinity Cache, 4 x 8 per XCD;
 *                  swizzle_stride ignored)
 *   "hgemm_auto"   kernel LC_HGEMM_AUTO launches on large 256-tileable shapes (a 256-tile lc_hgemm_variant value)
 *   "fp8_mx"       fp8 GEMM (lc_gemm_fp8_e4m3): 3 = MX-scaled K = 128 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4), generated loop (default);
 *                  1 = MX K = 64 MFMA, compiler-scheduled 4-wave kernel (the cross-check); 2 = MX K = 64, 8-wave kernel; 0 = plain K = 16
 *   "attn_d512"    D = 256 / 512 / 1024 kernel: 0 = auto (D = 256, N % 256 == 0, either V layout: 64 query rows per wave on v_mfma_f32_16x16x32 with K / V
 *                  rings, attn_bigd7.hip; D = 512: the full-width kernel on the same MFMA shape, attn_bigd6.hip; D = 256 with
 *                  N % 256 == 128: attn_bigd2.hip; D = 1024: two waves share 32 query rows and split the head dim, attn_bigd4.hip),
 *                  1 = round-1 column-split kernel, 2 = 32-row double-buffered tiles (attn_bigd3.hip: validated on hardware in round 3,
 *                  6-8 % slower, a cross-check), 3 = D = 256 / 512 on the other MFMA shape than auto (attn_bigd2.hip: v_mfma_f32_32x32x16),
 *                  4 = auto, but attn_bigd7 also on grids that do not fill the GPU (auto hands D = 256 launches of fewer than about 0.75
 *                  workgroups of 256 query rows per CU to attn_bigd2.hip, whose workgroups own 128 rows; lc_attn_kernel_name reports the
 *                  kernel of a grid that fills the GPU, lc_attn_kernel_name_bh the one a launch of BH problems runs)
 * Diagnosis keys (include/lc_diag.h) are rejected with LC_ERR_ARG unless the library was built with LC_DIAG=1. */
int lc_tune_set(const char* key, int value);
/* Current and default value of a knob (either pointer may be NULL); LC_ERR_ARG for an unknown key.  lc_tune_count / lc_tune_key
 * enumerate the keys (NULL for a diagnosis key in a production library).  The knobs are process-wide atomics: setting one while
 * another host thread launches is well defined (that launch sees the old or the new value), but A/B benches should not rely on it. */
int lc_tune_get(const char* key, int* value, int* default_value);
int lc_tune_count(void);
const char* lc_tune_key(int index);
/* Measures the constants of the split-KV launch rule on the CURRENT device (microseconds per KV tile at D = 128 / 64, fixed cost of the
 * combine launch, bytes per microsecond of partial traffic: about 60 tiny launches on zero-filled scratch, a few milliseconds) and makes
 * the rule use them for this device from now on; the built-in constants (fitted on the round-5 boxes) stay when this is never called or when
 * the measurement lies outside [0.4, 2.5] x of them (LC_ERR_ARG; out4 still receives what was measured).  out4 (optional): tau128, tau64,
 * x0_us, bytes_per_us.  bench.py calls it once per process; a caller that never does gets round 5's behaviour.  Not while `stream` is
 * being captured.  Knobs: "attn_calib" = 1 ignores the measurement; "rule_cus" = n makes every launch RULE (not the grids) reason with n
 * CUs instead of the device's own — for tests of the rules (64 .. 1024; 0 = the device). */
int lc_tune_calibrate(void* stream, float* out4);

/* Internal workspace (split-KV attention partials, split-K border strips of the GEMM): one cached device buffer per
 * (device, stream), grown geometrically, at most 16 per device and 1 GiB each; requests beyond that and launches on a stream that is
 * being captured run the workspace-free form of the same computation.  lc_workspace_bytes: bytes currently cached over all devices;
 * lc_workspace_release: hipFree every cached buffer (waits for the devices), returns the bytes given back — for callers that want
 * the memory back after a phase of small-grid launches.  Neither has a reference counterpart (its kernels allocate nothing). */
size_t lc_workspace_release(void);
size_t lc_workspace_bytes(void);

/* ---- HGEMM ------------------------------------------------------------------------------------
 * Replaces the host launchers + kernels of kernels/hgemm/mma/basic/hgemm_mma_stage.cu:644-1052,2284-2412
 * (NN) and kernels/hgemm/mma/swizzle/hgemm_mma_stage_tn_swizzle_x4.cu:207,892 (TN).
 * fp16 in, fp32 MFMA accumulate, fp16 out; no alpha/beta.
 * `stages` (2..5 in the reference, anything else falls back to 2: hgemm_mma_stage.cu:2388-2391) is ACCEPTED AND
 * IGNORED: the LDS ring depth is a fixed property of each kernel family here (2-slot rings; 2 + 3 slots for the W4
 * kernels that fill the CU's 160 KiB) — results never depend on it, exactly as in the reference.
 * `swizzle_stride` is the reference's thread-block-swizzle N-panel width in columns (hgemm.py:198-208): <= 1 means no
 * panel rasterisation.  Shapes: the tuned variants need M, N multiples of 256 (128 for MFMA128), K a multiple of 64
 * and 16-byte aligned pointers, else LC_ERR_SHAPE; LC_HGEMM_AUTO and LC_HGEMM_GENERIC accept ANY positive M, N, K and
 * 2-byte alignment (the edge-predicated kernel serves what the tiles do not divide; all address arithmetic is 64-bit). */
int lc_hgemm_f16(const void* A, const void* B, void* C, int M, int N, int K, int layout,
                 int variant, int stages, int swizzle_stride, void* stream);

/* Vendor comparator = the reference's cuBLAS entry points (kernels/hgemm/cublas/hgemm_cublas.cu:15-68,
 * 196-229) on hipBLASLt: init/destroy of a process-global handle + NN/TN GEMM, fp32 compute. */
int lc_vendor_init(void);
int lc_vendor_destroy(void);
int lc_hgemm_vendor_f16(const void* A, const void* B, void* C, int M, int N, int K, int layout,
                        void* stream);

/* EXTENSION (BASELINE config 5, no reference counterpart — the reference wrappers hard-require kHalf):
 * fp8 GEMM, OCP e4m3fn inputs, fp32 MFMA accumulate, fp16 output:  C[M,N] = alpha * A8[M,K] * B8^T with B8
 * stored [N,K] (the TN layout).  M, N multiples of 256, K multiple of 128, 16-byte aligned pointers. */
int lc_gemm_fp8_e4m3(const void* A, const void* B, void* C, int M, int N, int K, float alpha,
                     int swizzle_stride, void* stream);

/* EXTENSION: the same GEMM on OCP MX data — every 32 consecutive k of every row of A and of B carry an E8M0 block scale
 * (value = e4m3 * 2^(scale - 127); scale 127 = 1.0, 255 = NaN per the MX spec):
 *   C[m][n] = alpha * sum_k A8[m][k] 2^(SA[m][k/32] - 127) * B8[n][k] 2^(SB[n][k/32] - 127)
 * The matrix core wants one scale byte per lane (row, k block) and instruction; lc_mxfp8_pack_scales reorders the natural
 * [rows][K/32] byte array S into the dword array P (rows * K / 32 bytes, 8-byte aligned) that lc_gemm_mxfp8 consumes — once per weight
 * matrix, per call for activations.  rows multiple of 256, K multiple of 128.  P's layout is an implementation detail
 * (leetcuda_amd/csrc/gemm_fp8_w4k.hip); treat it as opaque. */
int lc_mxfp8_pack_scales(const void* S, void* P, int rows, int K, void* stream);
int lc_gemm_mxfp8(const void* A, const void* PA, const void* B, const void* PB, void* C, int M, int N, int K, float alpha,
                  int swizzle_stride, void* stream);

/* Dispatch by the reference's export name (hgemm.cc:126-181). 3-argument entries ignore
 * stages/swizzle/swizzle_stride. `init_cublas_handle` / `destroy_cublas_handle` take no tensors
 * (pass NULLs and zeros). */
int lc_hgemm_call(const char* entry, const void* A, const void* B, void* C, int M, int N, int K,
                  int stages, int swizzle, int swizzle_stride, void* stream);
int lc_hgemm_entry_count(void);
const char* lc_hgemm_entry_name(int index);
/* layout (lc_layout), number of reference arguments (0, 3 or 6); returns LC_ERR_ARG if unknown. */
int lc_hgemm_entry_info(const char* entry, int* layout, int* nargs);

/* ---- FlashAttention-2 forward -------------------------------------------------------------------
 * Replaces kernels/flash-attn/mma/basic/flash_attn_mma_split_q.cu:55,702,769,
 * flash_attn_mma_share_qkv.cu:70,772,872, flash_attn_mma_tiling_qkv.cu:75,800,881 and siblings.
 * Q,K,O: [B,H,N,D] fp16 contiguous.  V: [B,H,N,D], or [B,H,D,N] when v_transposed != 0
 * (the reference's *_swizzle_qkv share_kv/share_qkv/tiling_qk entries, flash_attn_mma.py:441-442).
 * Non-causal (causal: lc_attn_fwd_f16_ex), scale = 1/sqrt(D), no dropout / mask / LSE output.  fp32 softmax, fp32 MFMA accumulate
 * (family / acc_f32 / stages are accepted for signature parity and select nothing; CDNA4 MFMA has no fp16-accumulate form).
 * Batch variance: the kernel — and with it the fp32 summation order, i.e. the low bits of O — depends on B x H and the CU count
 * for shapes whose grid would not fill the GPU (small grids run 128-row workgroups or the split-KV path); one (B, H, N, D) on one
 * device is bit-reproducible from launch to launch.
 * N must be a multiple of 64; D in {32, 64, 96, 128, 256, 512, 1024} — the head dims of the reference dispatchers. */
int lc_attn_fwd_f16(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                    int v_transposed, int family, int acc_f32, int stages, void* stream);

/* EXTENSION (the reference has no causal mask): flags select the V layout and a causal mask.
 *   LC_ATTN_CAUSAL: query row i attends to key rows j <= i of the same (batch, head) (Q and K have the same length N).  fp16,
 *   D in {32, 64, 96, 128}, N % 64 == 0; other head dims give LC_ERR_HEADDIM.  One kernel, no workspace (legal under graph
 *   capture); D = 64 / 128 with N % 256 == 0 run attn_fwd_w4u_causal_kernel, the rest attn_fwd_causal_kernel.  The result does not
 *   depend on B x H, the CU count or the grid order ("attn_causal_order").
 *   Without LC_ATTN_CAUSAL the call is lc_attn_fwd_f16 (same plan, kernel and bits).  Unknown flag bits: LC_ERR_ARG. */
#define LC_ATTN_CAUSAL 1       /* key j visible to query i iff j <= i */
#define LC_ATTN_V_TRANSPOSED 2 /* V as [B,H,D,N] */
int lc_attn_fwd_f16_ex(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                       int flags, void* stream);

/* EXTENSION (the reference has one head count): grouped-query / multi-query attention.  Q, O: [B,H,N,D]; K: [B,Hkv,N,D]; V: [B,Hkv,N,D],
 * or [B,Hkv,D,N] with LC_ATTN_V_TRANSPOSED; G = H / Hkv.  Query head h of batch b attends to K / V head h / G of batch b (the
 * repeat_interleave convention of torch SDPA enable_gqa and flash-attn) — the result is, bit for bit, what lc_attn_fwd_f16_ex returns
 * on K and V expanded G times along the head axis, without the copy.  flags, scale, causal mask and softmax as lc_attn_fwd_f16_ex.
 *   Hkv == H: the call IS lc_attn_fwd_f16_ex (same plan, kernel and bits; every head dim that entry takes).
 *   Hkv <  H: fp16, D in {32, 64, 96, 128}, N % 64 == 0, causal or not, both V layouts; D >= 256 gives LC_ERR_HEADDIM (no grouped-query
 *   kernels for the large head dims yet).  Hkv < 1, Hkv > H or H % Hkv != 0: LC_ERR_SHAPE.  Checks in lc_attn_fwd_f16_ex's order
 *   (flags / null pointer: LC_ERR_ARG, then shape, then head dim), all before any device work.
 *   The plan is the one lc_attn_fwd_f16_ex makes for the same (B x H, N, D, flags) — kernel family, walk, split-KV factor, waves, causal
 *   grid order; nothing is decided by Hkv — and the kernel is that plan's kernel under the name with `_kernel` replaced by
 *   `_gqa_kernel` (attn_fwd_w4u_gqa_kernel<128,false,1>, attn_fwd_w4u_causal_gqa_kernel<64,true>, attn_fwd_w4i_gqa_kernel<96,1>,
 *   attn_fwd_gqa_kernel<...>, attn_fwd_causal_gqa_kernel<...>): the batch-variance note above and every lc_tune_set knob apply unchanged.
 * lc_attn_kernel_name_gqa(BH = B x H query heads or <= 0, G, ...) never launches; G == 1: lc_attn_kernel_name_ex's answer; G < 1 or
 * BH > 0 with BH % G != 0: LC_ERR_SHAPE. */
int lc_attn_fwd_f16_gqa(const void* Q, const void* K, const void* V, void* O, int B, int H, int Hkv, int N, int D,
                        int flags, void* stream);
int lc_attn_kernel_name_gqa(int BH, int G, int N, int D, int flags, char* buf, int buflen);

/* EXTENSION: attention of Nq new query tokens per sequence over a KV cache (decode; attn_decode.hip).
 * Q, O: [B,H,Nq,D] fp16.  K, V: [B,Hkv,Ncap,D] fp16 — the cache, Ncap = its capacity in tokens (any value >= 1).
 * kv_len: DEVICE int32[B], number of valid cache positions of each batch entry (the Nq new tokens already appended), or NULL = Ncap for all.
 * Read by the kernel, never by the host: a captured graph may be replayed after the array was changed in place.  Values are clamped to
 * [0, Ncap] in the kernel.
 * G = H / Hkv; query head h reads K / V head h / G (the convention of lc_attn_fwd_f16_gqa).
 * Without LC_ATTN_CAUSAL every query sees keys 0 .. L_b - 1.  With it, query i sees keys j <= L_b - Nq + i (bottom-right aligned: the last
 * query sees the whole cache; the flash-attn kv-cache convention).  A row with no visible key (L_b == 0, or causal with L_b - Nq + i < 0)
 * gets O = 0.  The result never depends on what the cache holds at positions >= L_b (NaN and Inf included).
 * workspace: NULL, or a caller-owned device buffer of at least lc_attn_decode_workspace_bytes(...) bytes, 16-byte aligned, that makes the
 * split-KV form legal while `stream` is being captured.  Without it the split-KV form keeps its partials in the stream's cached workspace
 * (lc_workspace_bytes); a stream that is being captured then runs the one-launch form (S = 1).
 * Restrictions: D in {64, 128} (else LC_ERR_HEADDIM); R = G x Nq query rows per K / V head, 1 <= R <= 64 (else LC_ERR_SHAPE: chunked
 * prefill against a cache is lc_attn_chunk_f16 below); LC_ATTN_V_TRANSPOSED and unknown flag bits: LC_ERR_ARG; Hkv < 1, Hkv > H, H % Hkv != 0,
 * non-positive dims, one head's Ncap x D x 2 >= 2 GiB, pointers not 16-byte aligned: LC_ERR_SHAPE.  Checks in lc_attn_fwd_f16_gqa's order
 * (flags / null pointer, then shape, then head dim; then a non-NULL workspace that is too small or not 16-byte aligned: LC_ERR_ARG), all
 * before any device work.
 * Kernel: attn_decode_kernel<D, RT> (RT = 1 / 2 / 4 row tiles of 16 hold the R rows), one workgroup per (batch, K / V head, KV range s of S);
 * S > 1: + attn_decode_combine_kernel<D> over fp32 partials.  S is chosen on the host from (B x Hkv, ceil(Ncap / 64), the CU count,
 * "attn_decode_split"), never from kv_len; each batch entry's ranges are cut in the kernel from its own L_b.
 * Reproducibility: the bits of one (batch, K / V head) depend on its Q, K, V, L_b, Nq, flags and S only — not on B, on the other batch
 * entries' lengths or on the grid position (compare the batch-variance note of lc_attn_fwd_f16: here only S depends on B, through the rule).
 * lc_attn_decode_workspace_bytes: what the current plan of that shape needs (0 for S = 1, and for a shape the call refuses).
 * lc_attn_decode_kernel_name never launches: the kernel's demangled name, with S > 1 followed by " xS" (the split-K HGEMM convention). */
int lc_attn_decode_f16(const void* Q, const void* K, const void* V, void* O, const int* kv_len,
                       int B, int H, int Hkv, int Nq, int Ncap, int D, int flags,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_decode_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int D);
int lc_attn_decode_kernel_name(int B, int H, int Hkv, int Nq, int Ncap, int D, int flags, char* buf, int buflen);

/* EXTENSION: lc_attn_decode_f16 over a PAGED KV cache addressed through a block table (attn_decode_paged.hip) — what a
 * serving loop that keeps its cache in fixed-size pages calls, with no gather in front.
 * Q, O: [B,H,Nq,D] fp16, as in lc_attn_decode_f16.
 * Kpool, Vpool: [num_pages,Hkv,page_size,D] fp16, dense: one (page, K / V head) is one contiguous run of page_size x D halves.  (A contiguous
 * [B,Hkv,Ncap,D] cache with Ncap a power of two IS a pool with num_pages = B, page_size = Ncap and the table [[0],[1],...]: no copy.)
 * block_table: DEVICE int32[B,max_pages], dense; entry [b][p] is the pool page that holds logical keys p page_size .. (p + 1) page_size - 1 of
 * batch entry b.  One table serves K and V and every K / V head.
 * kv_len: DEVICE int32[B], required.  The logical capacity is Ncap = max_pages x page_size; kv_len is clamped to [0, Ncap] in the kernel.
 * Only the kernel reads block_table and kv_len, never the host: a captured graph may be replayed after either was rewritten in place.
 * Flags, the bottom-right causal convention, "a row without a visible key gets O = 0", R = (H / Hkv) x Nq <= 64 and D in {64, 128} are those of
 * lc_attn_decode_f16.
 * Never read: table entries at positions >= ceil(L_b / page_size), and pool rows that hold logical positions >= L_b; the result depends on
 * neither (NaN and Inf included).
 * MEMORY SAFETY: the host cannot check the table.  The kernel clamps every page id it reads to [0, num_pages - 1] before use — a garbage entry
 * reads a wrong page, never an address outside the pool — and that clamp is the whole of the memory-safety story: num_pages must be the true
 * page count of BOTH pools.
 * page_size: a power of two >= 16 (else LC_ERR_SHAPE); one (page, head) run below 2 GiB.  The pool as a whole may exceed 4 GiB (64-bit page
 * base, 32-bit offset inside a run).
 * Checks, in lc_attn_decode_f16's order and all before any device work: unknown flags or a NULL Q / Kpool / Vpool / O / block_table / kv_len:
 * LC_ERR_ARG; then LC_ERR_SHAPE for H % Hkv, non-positive B / Nq / num_pages / max_pages / D, a bad page_size, R > 64, max_pages x page_size x
 * D x 2 >= 2 GiB, the grid bound, Q / O / pools not 16-byte aligned; then D not in {64, 128}: LC_ERR_HEADDIM; then a non-NULL workspace that is
 * too small or not 16-byte aligned: LC_ERR_ARG.
 * Kernel: attn_decode_paged_kernel<D, RT>, S > 1: + attn_decode_combine_kernel<D>; S, the workspace bytes and the capture / failed-lease
 * fallback to S = 1 are those of lc_attn_decode_f16 at Ncap = max_pages x page_size (same rule, same "attn_decode_split", same CU count).
 * For the same Q, logical cache contents, kv_len, flags and S the output is BIT-IDENTICAL to lc_attn_decode_f16 on the gathered contiguous
 * cache of that Ncap: paging changes where a row comes from and nothing about the arithmetic.
 * The name call never launches: "attn_decode_paged_kernel<D,RT>", with S > 1 followed by " xS". */
int lc_attn_decode_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O,
                             const int* block_table, const int* kv_len,
                             int B, int H, int Hkv, int Nq,
                             int num_pages, int page_size, int max_pages, int D, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_decode_paged_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D);
int lc_attn_decode_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D,
                                     int flags, char* buf, int buflen);

/* EXTENSION: lc_attn_decode_paged_f16 over a paged KV cache kept in fp8 (attn_decode_paged_kv8.hip): the call is bound
 * by reading K and V once, and this halves what is read.
 *   O = softmax(Q (k_scale[g] K8)^T / sqrt(D)) (v_scale[g] V8),   g = the K / V head of the query head
 * Q, O, block_table, kv_len, flags, workspace and stream are exactly those of lc_attn_decode_paged_f16.
 * Kpool8, Vpool8: [num_pages,Hkv,page_size,D] bytes, each an OCP e4m3fn value (the format of lc_gemm_fp8_e4m3 and of torch.float8_e4m3fn: bias
 * 7, no infinity, 0x7f / 0xff = NaN), dense and 16-byte aligned.
 * k_scale, v_scale: DEVICE float[Hkv], one scale per K / V head, or NULL = 1.0.  Like block_table and kv_len they are read by the kernel only: a
 * captured graph may be replayed after they were rewritten in place.  They are applied in fp32 (k_scale inside the score scale, v_scale inside
 * the normalisation of O), never to an fp16 value.
 * The mask, the clamps of kv_len and of page ids, "a row without a visible key gets O = 0" and what is never read (table entries at positions >=
 * ceil(L_b / page_size), pool bytes of positions >= L_b — NaN codes included) are those of lc_attn_decode_paged_f16; so is the memory-safety note.
 * Checks: lc_attn_decode_paged_f16's, in its order, with the two fp8 pools in the pointer and alignment checks; k_scale / v_scale may be NULL and
 * are not checked.  The span bound is that of one-byte elements: max_pages x page_size x D >= 2 GiB is LC_ERR_SHAPE.
 * Kernel: attn_decode_paged_kv8_kernel<D, RT>, S > 1: + attn_decode_combine_kernel<D>.  RT, S, the workspace bytes and the capture / failed-lease
 * fallback to S = 1 are those of lc_attn_decode_paged_f16 for the same shape (same rule, same "attn_decode_split", same CU count).
 * Every e4m3 value is an fp16 value and the kernel converts exactly, so with power-of-two scales that keep the dequantised values normal fp16
 * numbers the output is BIT-IDENTICAL to lc_attn_decode_paged_f16 on the dequantised fp16 pool (same Q, table, kv_len, flags and S).
 * Not here: a contiguous fp8 entry (a contiguous cache with Ncap a power of two is a pool with num_pages = B), per-token or per-page scales,
 * e5m2, fp8 Q.  (What writes these pools: lc_kv_append_paged_kv8 below.)
 * The name call never launches: "attn_decode_paged_kv8_kernel<D,RT>", with S > 1 followed by " xS". */
int lc_attn_decode_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O,
                             const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                             int B, int H, int Hkv, int Nq,
                             int num_pages, int page_size, int max_pages, int D, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_decode_paged_kv8_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D);
int lc_attn_decode_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D,
                                         int flags, char* buf, int buflen);

/* EXTENSION: the write side of the paged KV cache (kv_append_paged.hip): the K and V rows of the Nq newest tokens of
 * every sequence go into the pools that lc_attn_decode_paged_f16 / lc_attn_decode_paged_kv8 read, through the same block table and the same
 * kv_len array, in ONE launch for K and V.  One decoding step is: bump kv_len on the device, append, decode — on one stream, capturable as one
 * graph.  A prefill is the same call with Nq = the prompt length.
 * Knew, Vnew: [B,Hkv,Nq,D] fp16, dense, 16-byte aligned: the rows of the Nq newest tokens.  Never written.
 * Kpool, Vpool (fp16) / Kpool8, Vpool8 (OCP e4m3fn bytes): [num_pages,Hkv,page_size,D], the layout of the decode calls, 16-byte aligned.
 * block_table: DEVICE int32[B,max_pages]; kv_len: DEVICE int32[B]; k_scale, v_scale (fp8 call): DEVICE float[Hkv], or NULL = 1.0.  All of them
 * are read by the kernel only, never by the host: a captured graph may be replayed after they were rewritten in place.
 * Where a token goes: kv_len[b] is the length AFTER the append — the value the decode call of the same step is handed.  L = kv_len[b] clamped to
 * [0, max_pages x page_size] (the decode kernels' clamp); token i of batch entry b has position p = L - Nq + i, the position the bottom-right
 * causal mask of lc_attn_decode_* gives query i.  p < 0: the token is not written, so a batch of LEFT-PADDED prompts of different lengths fills
 * its caches in one call with Nq = the longest prompt.  Otherwise it goes to page block_table[b][p / page_size], row p % page_size, of every
 * K / V head.  A page id outside [0, num_pages) DROPS the token — unlike the read side, which clamps: a write to a clamped page would corrupt
 * another sequence's cache.  Table entries of pages that hold none of the Nq positions are never read.  Nothing but the target rows of the two
 * pools is written (Hkv x D elements per written token and pool).  Two batch entries that name the same page and row: which one lands is
 * unspecified.
 * MEMORY SAFETY: as on the read side the host cannot check the table; num_pages must be the true page count of BOTH pools.
 * fp8: the code of element x of K / V head g is e4m3fn_rne(clamp(fp32(x) / scale[g], -448, 448)): the fp32 quotient is the correctly rounded
 * IEEE division (not a multiplication by a reciprocal), the conversion rounds to nearest even onto e4m3fn, subnormals included; +-inf gives
 * +-448, -0 gives 0x80, NaN gives a NaN code (code & 0x7f == 0x7f).  Scales are expected positive and finite.
 * Checks, all before any device work: flags != 0 (no flag is defined), then a NULL Knew / Vnew / pool / block_table / kv_len: LC_ERR_ARG; then
 * LC_ERR_SHAPE for non-positive B / Hkv / Nq / num_pages / max_pages / D, page_size not a power of two >= 16, max_pages x page_size not an
 * int, max_pages x page_size x D x (element bytes) >= 2 GiB (the decode calls' bound: every pool geometry append accepts, decode accepts), a
 * grid of B x Hkv x ceil(Nq D / 2048) workgroups that does not fit an int, Knew / Vnew / pools not 16-byte aligned; then D not in {64, 128}:
 * LC_ERR_HEADDIM.  Nq is NOT bounded by the decode kernels' 64 rows: a prefill writes whole prompts.  No workspace.
 * Kernels: kv_append_paged_kernel<D>, kv_append_paged_kv8_kernel<D>.  The name calls never launch, take no num_pages (it decides nothing) and
 * return the status the run call gives that shape; a NULL buffer or buflen < 8: LC_ERR_ARG.
 * Not here: per-token or per-page scales, pools laid out [P,page_size,Hkv,D], an append to a contiguous cache, ragged Nq per sequence other
 * than by left padding (a ragged batch: lc_rope_append_varlen_* below, which a table of cos = 1, sin = 0 makes a plain append).  (A
 * token-major [B,Nq,Hkv,D] source and rotary embedding: lc_rope_append_paged_* below.)
 * bfloat16: for 16-bit pools lc_kv_append_paged_f16 is a copy of bits and serves bf16 rows and pools as it stands (the pools that
 * lc_attn_varlen_paged_bf16 reads); there is no bf16 form of lc_kv_append_paged_kv8 — lc_rope_append_varlen_kv8_bf16 with a table of cos = 1,
 * sin = 0 quantises bf16 rows. */
int lc_kv_append_paged_f16(const void* Knew, const void* Vnew, void* Kpool, void* Vpool,
                           const int* block_table, const int* kv_len,
                           int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D,
                           int flags, void* stream);
int lc_kv_append_paged_kv8(const void* Knew, const void* Vnew, void* Kpool8, void* Vpool8,
                           const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                           int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D,
                           int flags, void* stream);
int lc_kv_append_paged_kernel_name(int B, int Hkv, int Nq, int page_size, int max_pages, int D,
                                   int flags, char* buf, int buflen);
int lc_kv_append_paged_kv8_kernel_name(int B, int Hkv, int Nq, int page_size, int max_pages, int D,
                                       int flags, char* buf, int buflen);

/* EXTENSION: rotary embedding (RoPE) fused with the append (rope_append_paged.hip): the link between the QKV projection
 * GEMM and lc_kv_append_paged_* / the attention calls.  ONE launch rotates Q and K by position, writes Q in the layout lc_attn_decode_* /
 * lc_attn_chunk_* read, and writes the rotated (fp8: quantised) K and the unrotated V into the pools — through the same block_table / kv_len
 * pair, so prefill -> append -> decode is a sequence of this library's calls only, capturable as one graph.
 * Positions are the append call's: L = kv_len[b] clamped to [0, max_pages x page_size] is the length AFTER the append, token i has position
 * p = L - Nq + i.  K and V of token i land where lc_kv_append_paged_* puts them (p < 0: no pool write; a page id outside [0, num_pages) drops the
 * token's K and V rows).  V is not rotated: the V pool is byte for byte what lc_kv_append_paged_f16 / _kv8 writes.
 * cos_sin: DEVICE float[max_pos, rot_dim]; row t holds cos(theta_{t,j}), j = 0 .. rot_dim/2 - 1, then sin(theta_{t,j}) for the same j (vLLM's
 * cos_sin_cache layout, in fp32).  The caller owns the angles (base, scaling, NTK, YaRN): the kernel does no trigonometry.  The row read for
 * position p is min(p, max_pos - 1): clamped in the kernel, nothing is read outside the table.
 * Rotation of a row x (a Q row of any of the H heads, a K row of any of the Hkv heads) at position p: pair j is elements (j, j + rot_dim/2)
 * (default: NeoX / Llama "rotate half") or (2j, 2j + 1) (LC_ROPE_INTERLEAVED: GPT-J); x1' = x1 c - x2 s, x2' = x2 c + x1 s.  Inputs go from fp16
 * to fp32, all arithmetic is fp32, ONE rounding to fp16 (nearest even) at the end; fp16 denormals are kept on input and output.  Elements
 * rot_dim .. D - 1 (partial rotary) are copied bit for bit.  A pair with a non-finite input has unspecified outputs; nothing outside it is
 * affected.
 * Qout: [B,H,Nq,D] fp16 dense, row (b, h, i) rotated at position p; rows with p < 0 are ZEROS; a dropped page id does not affect Qout.
 * fp16 pools get the rotated fp16 K row; fp8 pools get lc_kv_append_paged_kv8's code of the rotated row ROUNDED TO fp16 FIRST, so the fp8 entry
 * equals, byte for byte, lc_kv_append_paged_kv8 fed with what the fp16 entry wrote.
 * Sources.  Default: Q [B,H,Nq,D], Knew and Vnew [B,Hkv,Nq,D], dense, src_row_stride = 0; Qout == Q (the same pointer) rotates in place.
 * LC_ROPE_PACKED_SRC: Q, Knew and Vnew point into ONE token-major projection output: element (b, i, h, d) of a source is at
 * ptr[(b Nq + i) src_row_stride + h D + d]; src_row_stride is in elements, a multiple of 8 and >= (H + 2 Hkv) D; a caller passes qkv,
 * qkv + H D and qkv + (H + Hkv) D.  Qout is still dense [B,H,Nq,D] (the call transposes too) and must not overlap the sources.
 * Checks, all before any device work: a flag bit other than the two defined, then a NULL Q / Knew / Vnew / Qout / pool / cos_sin / block_table /
 * kv_len: LC_ERR_ARG; then LC_ERR_SHAPE for non-positive B / H / Hkv / Nq / num_pages / max_pages / D / max_pos, H % Hkv != 0, the append call's
 * page and span bounds, rot_dim not a multiple of 16 in [16, D], src_row_stride != 0 without LC_ROPE_PACKED_SRC or (with it) not a multiple of 8
 * or < (H + 2 Hkv) D, a grid of (B Hkv + B H) x ceil(Nq D / 2048) workgroups that does not fit an int, Q / Knew / Vnew / Qout / pools not
 * 16-byte aligned; then D not in {64, 128}: LC_ERR_HEADDIM.  Nq is unbounded, there is no workspace.
 * Kernels: rope_append_paged_kernel<D,INTERLEAVED>, rope_append_paged_kv8_kernel<D,INTERLEAVED>.  The name calls never launch, take no
 * num_pages and return the status the run call gives that shape; a NULL buffer or buflen < 8: LC_ERR_ARG.
 * Not here: explicit per-token position ids (tree speculation, M-RoPE), an fp16 / bf16 table or angles computed in the kernel, bf16 sources
 * (the ragged form has them: lc_rope_append_varlen_bf16 / _kv8_bf16 below), RoPE for the contiguous cache, D outside {64, 128}. */
#define LC_ROPE_INTERLEAVED 1
#define LC_ROPE_PACKED_SRC 2
int lc_rope_append_paged_f16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                             const float* cos_sin, const int* block_table, const int* kv_len,
                             int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D,
                             int rot_dim, int max_pos, long long src_row_stride, int flags, void* stream);
int lc_rope_append_paged_kv8(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8,
                             const float* cos_sin, const int* block_table, const int* kv_len,
                             const float* k_scale, const float* v_scale,
                             int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D,
                             int rot_dim, int max_pos, long long src_row_stride, int flags, void* stream);
int lc_rope_append_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D,
                                     int rot_dim, int max_pos, long long src_row_stride, int flags, char* buf, int buflen);
int lc_rope_append_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D,
                                         int rot_dim, int max_pos, long long src_row_stride, int flags, char* buf, int buflen);

/* EXTENSION: chunked-prefill attention over the three KV caches (attn_chunk.hip): lc_attn_decode_f16,
 * lc_attn_decode_paged_f16 and lc_attn_decode_paged_kv8 with the bound R = (H / Hkv) x Nq <= 64 REMOVED — what attends over a chunk of a prompt
 * that lc_kv_append_paged_* just wrote (chunked prefill, prefill behind a shared or cached prefix, speculative verification with many draft
 * tokens, MQA with G = 64 and Nq >= 2), with no gather of the pages and no mask built by hand.
 * Every argument, argument for argument, is that of the decode entry of the same cache kind, and so is everything its comment says: Q, O
 * [B,H,Nq,D] fp16; kv_len is the length AFTER the chunk was appended; LC_ATTN_CAUSAL is bottom-right aligned (query i sees keys j <= L_b - Nq + i);
 * a row with no visible key gets O = 0; D in {64, 128}; page ids are clamped in the kernel; nothing is read at logical positions >= L_b or in
 * table entries at positions >= ceil(L_b / page_size); the workspace rules and the capture / failed-lease fallback to S = 1; the checks and
 * their order, with ONE difference: R > 64 is not an error (R is computed in 64 bits), and the grid bound is B x Hkv x RB x 64 <= 2^31 - 1 with
 * RB = ceil(R / 64).
 * R <= 64 through a chunk entry IS the decode call: same plan, same kernel name, same bits.  A caller needs one call site.
 * R > 64: attn_chunk_kernel<D> / attn_chunk_paged_kernel<D> / attn_chunk_paged_kv8_kernel<D> (four row tiles of 16, the decode body) on
 * B x Hkv x RB x S workgroups, block rb of a (batch, K / V head) owning rows 64 rb .. of its [R,D] matrix; S > 1: + attn_decode_combine_kernel<D>
 * over S x B H Nq x (D + 1) floats.  S follows the decode rule with B x Hkv x RB groups; "attn_decode_split" forces it.  With LC_ATTN_CAUSAL a
 * block walks only the keys some row of it can see (below L_blk = clamp(L_b - Nq + i_max + 1, 0, L_b), i_max the block's last token, Nq - 1
 * where the block straddles a head boundary): a block of a call with Nq % 64 == 0 computes, bit for bit, what the decode call computes on its
 * 64 query rows with kv_len = L_blk.  The bit-identity notes of the paged and fp8 decode calls (against the gathered / dequantised cache at equal
 * S) hold for the chunk calls.
 * Each row block streams its visible K / V again (only L2 shares the reads): expect a rate well below lc_attn_fwd_f16_gqa's causal kernel at
 * large Nq; the call serves what that kernel cannot (Nq != Nk, paged and fp8 caches).
 * The name calls never launch: R > 64: "attn_chunk_kernel<D>", "attn_chunk_paged_kernel<D>", "attn_chunk_paged_kv8_kernel<D>", with S > 1
 * followed by " xS"; R <= 64: the decode entry's name. */
int lc_attn_chunk_f16(const void* Q, const void* K, const void* V, void* O, const int* kv_len,
                      int B, int H, int Hkv, int Nq, int Ncap, int D, int flags,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_chunk_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int D);
int lc_attn_chunk_kernel_name(int B, int H, int Hkv, int Nq, int Ncap, int D, int flags, char* buf, int buflen);
int lc_attn_chunk_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O,
                            const int* block_table, const int* kv_len,
                            int B, int H, int Hkv, int Nq,
                            int num_pages, int page_size, int max_pages, int D, int flags,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_chunk_paged_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D);
int lc_attn_chunk_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D,
                                    int flags, char* buf, int buflen);
int lc_attn_chunk_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O,
                            const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                            int B, int H, int Hkv, int Nq,
                            int num_pages, int page_size, int max_pages, int D, int flags,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_chunk_paged_kv8_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D);
int lc_attn_chunk_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D,
                                        int flags, char* buf, int buflen);

/* EXTENSION: sliding-window and attention-sink attention over the three KV caches (attn_local.hip): the chunk entries
 * above with two more arguments in front of `flags`, for models whose layers attend to the last W keys only (Mistral-class, Gemma 2 / 3,
 * gpt-oss) and whose heads carry a learned sink logit (gpt-oss).  Neither can be had from outside: the low edge of a window moves per query
 * row, and a sink changes the softmax denominator inside the kernel.
 *   window  W > 0: query i of batch entry b, at position p = L_b - Nq + i, sees keys j with p - W < j <= p: W keys including its own (the
 *           Hugging Face `sliding_window` convention; FlashAttention's window_size = (W - 1, 0)), the low edge clipped at key 0.  0: no low
 *           edge.  W < 0, and W > 0 without LC_ATTN_CAUSAL: LC_ERR_ARG.
 *   sinks   device float[H] or NULL, read by the kernel only (never by the host: the call stays graph-capturable, and a replay sees the
 *           values of its time).  sinks[h] is a logit in natural units — it is NOT multiplied by 1 / sqrt(D) — of every row of query head h:
 *           exp(sinks[h] - max) is added to the softmax denominator, nothing to the numerator.  -inf is no sink; +inf and NaN are not
 *           supported.  Allowed with or without a window, causal or not.  A row with a sink and no visible key gets O = 0, as without one.
 * Everything else is the chunk entries', word for word: Q, O [B,H,Nq,D] fp16, the kv_len clamp, the page-id clamp, the scales, alignment, the
 * 2 GiB span bounds, D in {64, 128}, R = (H / Hkv) x Nq unbounded, the workspace rules and the capture / failed-lease fallback to S = 1.  The
 * checks are the chunk entries' in their order, the two new LC_ERR_ARG cases right behind the unknown-flag check, all before any device work.
 * window == 0 && sinks == NULL IS the chunk call: same plan, same kernel name, same bits.
 * Otherwise: attn_local_kernel<D,RT> / attn_local_paged_kernel<D,RT> / attn_local_paged_kv8_kernel<D,RT> (R <= 64) or attn_local_chunk_kernel<D> /
 * attn_local_chunk_paged_kernel<D> / attn_local_chunk_paged_kv8_kernel<D> (R > 64) on the grid of the decode / chunk kernel of that shape.  With
 * a window a workgroup starts at the 64-key tile of the lowest key one of its rows sees, tile_lo = max(0, L_b - Nq + i_min + 1 - W) / 64
 * (i_min: its lowest token; 0 for R <= 64 and for a row block that straddles a head boundary), and it is the tiles [tile_lo, T) that are cut
 * into the S ranges: cache rows below tile_lo x 64 and block-table entries below that position are never read, and the time follows W, not L_b.
 * A call with Nq = 1 whose L_b - W is a multiple of 64 computes, bit for bit, what the decode call computes on cache rows [L_b - W, L_b) with
 * kv_len = W at equal S.  S never depends on kv_len: it follows the decode rule with the tiles of min(Ncap, W + Nq - 1 + 63) keys in place of
 * those of Ncap when W > 0; "attn_decode_split" forces it; the workspace is S x B H Nq x (D + 1) floats as before.
 * The two query calls take `window` and no sinks: S and the bytes do not depend on sinks; the name call reports the kernel of a call WITHOUT
 * sinks (window = 0: the chunk call's name) — with sinks the kernel is the attn_local_* one of the same template arguments and S. */
int lc_attn_local_f16(const void* Q, const void* K, const void* V, void* O, const int* kv_len,
                      int B, int H, int Hkv, int Nq, int Ncap, int D, int window, const float* sinks, int flags,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_local_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int D, int window);
int lc_attn_local_kernel_name(int B, int H, int Hkv, int Nq, int Ncap, int D, int window, int flags, char* buf, int buflen);
int lc_attn_local_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O,
                            const int* block_table, const int* kv_len,
                            int B, int H, int Hkv, int Nq,
                            int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_local_paged_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window);
int lc_attn_local_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window,
                                    int flags, char* buf, int buflen);
int lc_attn_local_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O,
                            const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                            int B, int H, int Hkv, int Nq,
                            int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_local_paged_kv8_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window);
int lc_attn_local_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window,
                                        int flags, char* buf, int buflen);

/* EXTENSION: ragged-batch (varlen) attention over the paged caches (attn_varlen.hip): the paged local entries above for a
 * continuous-batching step, whose sequences bring different numbers of new tokens — a few prompts or one prefill chunk next to many sequences
 * that decode one token.  The step is stated once: its tokens are packed token-major, one sequence behind the other, and cu_q holds the offsets
 * (FlashAttention's flash_attn_varlen_func with a block table).  There is no contiguous-cache form: a ragged batch only exists on a paged cache.
 *   Q, O    token-major [T, H, D] fp16: row t, head h at (t H + h) D — what lc_rope_append_varlen_* below writes.
 *   cu_q    device int32[B + 1], read by the kernel only (never by the host, like kv_len: the call stays graph-capturable and a replay sees
 *           the offsets of its time).  Sequence b owns rows q0 = clamp(cu_q[b], 0, T) ... q0 + Nq_b - 1 with
 *           Nq_b = clamp(cu_q[b + 1] - q0, 0, min(max_nq, T - q0)).  The clamps are the memory-safety contract, like the page-id clamp: NO value
 *           in cu_q makes a kernel read or write outside the T rows.  Nq_b = 0 is legal and does no work.  Rows at or past cu_q[B] (below T)
 *           and rows below cu_q[0] are NOT written, whether the plan has one KV range or several.  (A row between the two that the clamps
 *           leave to no sequence — cu_q not monotone, a sequence longer than max_nq — is not written with one KV range and holds an
 *           unspecified value with several.)
 *   T       host upper bound: the rows of Q and O.   max_nq   host upper bound: the largest Nq_b the caller will ever put in cu_q.
 * kv_len[b] is the length AFTER the step's append: query i of sequence b sits at position p = L_b - Nq_b + i.  LC_ATTN_CAUSAL, window, sinks,
 * the scales, the kv_len and page-id clamps, D in {64, 128}, the alignment and the span rules are lc_attn_local_paged_*'s, word for word.
 * The checks are that entry's in its order; a NULL cu_q joins the NULL-pointer check (LC_ERR_ARG); T < 1, max_nq < 1 and max_nq > T join the
 * shape check (LC_ERR_SHAPE).
 * Plan: G = H / Hkv, RB = ceil(G max_nq / 64); B x Hkv x RB x S workgroups, of which one whose row block starts at or past G Nq_b returns at
 * once.  RB = 1: attn_varlen_paged_kernel<D,RT> / attn_varlen_paged_kv8_kernel<D,RT> with the RT of the decode plan of R = G max_nq; RB > 1:
 * attn_varlen_chunk_paged_kernel<D> / attn_varlen_chunk_paged_kv8_kernel<D>; window = 0 and sinks = NULL run the same kernels.  Inside a
 * (sequence, K / V head) the rows are ordered as in the rectangular call: a ragged call whose Nq_b all equal max_nq computes, bit for bit,
 * what lc_attn_local_paged_* computes at equal S on the same tokens as [B,H,Nq,D].  S never depends on device data: the decode rule with
 * Hkv x min(B RB, ceil(G T / 64) + B) groups, and with W > 0 the tiles of min(Ncap, W + max_nq - 1 + 63) keys; "attn_decode_split" forces it.
 * S > 1 is followed by attn_varlen_combine_kernel<D>.  The workspace is S x T H x (D + 1) floats, the workspace rules and the capture /
 * failed-lease fallback to S = 1 are the other decode entries'.  The query calls take no sinks and no pointers. */
int lc_attn_varlen_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O,
                             const int* cu_q, const int* block_table, const int* kv_len,
                             int B, int H, int Hkv, int T, int max_nq,
                             int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_varlen_paged_workspace_bytes(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window);
int lc_attn_varlen_paged_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                     int flags, char* buf, int buflen);
int lc_attn_varlen_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O,
                             const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                             int B, int H, int Hkv, int T, int max_nq,
                             int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);
size_t lc_attn_varlen_paged_kv8_workspace_bytes(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window);
int lc_attn_varlen_paged_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                         int flags, char* buf, int buflen);

/* EXTENSION: rotary embedding + append for a ragged batch (rope_append_varlen.hip): lc_rope_append_paged_* for the
 * step that lc_attn_varlen_paged_* reads, with the same cu_q, T and max_nq and the same clamps.
 *   Q, Knew, Vnew   token-major fp16 with a row stride each, in elements: element (t, h, d) of Q at Q[t q_row_stride + h D + d], of Knew / Vnew
 *           at ptr[t kv_row_stride + h D + d].  Both strides are multiples of 8, q_row_stride >= H D, kv_row_stride >= Hkv D.  Three pointers
 *           into one projection output [T, (H + 2 Hkv) D] are the usual case, dense [T,H,D] and [T,Hkv,D] the other.  LC_ROPE_PACKED_SRC is
 *           NOT accepted (LC_ERR_ARG): the strides say it all.
 *   Qout    dense [T,H,D] fp16; may be Q itself when q_row_stride == H D (else LC_ERR_SHAPE).
 * Token t belongs to the sequence b with cu_q[b] <= t < cu_q[b + 1] under the clamps above; its position is p = L_b - Nq_b + (t - q0).
 * Everything else is lc_rope_append_paged_*'s rule, by the same device functions: p < 0 (no pool write, a zero row in Qout), a bad page id,
 * the table-row clamp, NeoX and GPT-J pairs, partial rotary, fp32 arithmetic with one rounding, the fp8 code of the row rounded to fp16.  A
 * token at or past cu_q[B], or one that the clamps leave to no sequence, writes NOTHING, in the pools or in Qout.
 * The grid is over global token blocks, ceil(T / (2048 / D)) x (Hkv + H) workgroups: it does not grow with B x max_nq; every row finds its
 * sequence by a binary search of cu_q.  Checks: lc_rope_append_paged_*'s in their order; a NULL cu_q is LC_ERR_ARG; T < 1, max_nq < 1,
 * max_nq > T and a bad stride are LC_ERR_SHAPE.  rope_append_varlen_kernel<D,INTERLEAVED> / rope_append_varlen_kv8_kernel<D,INTERLEAVED>.
 * There is no ragged plain append yet: a table of cos = 1, sin = 0 makes this call one. */
int lc_rope_append_varlen_f16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                              const float* cos_sin, const int* cu_q, const int* block_table, const int* kv_len,
                              int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                              int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_kv8(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8,
                              const float* cos_sin, const int* cu_q, const int* block_table, const int* kv_len,
                              const float* k_scale, const float* v_scale,
                              int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                              int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                      int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                      char* buf, int buflen);
int lc_rope_append_varlen_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                          int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                          char* buf, int buflen);

/* EXTENSION: bfloat16 forms of the four ragged entries above (attn_varlen_bf16.hip, rope_append_varlen_bf16.hip) — what a
 * model that ships in bfloat16 (Llama 3, Mistral, Gemma 2 / 3, gpt-oss) needs for one serving step: [GEMM -> lc_rope_append_varlen_bf16 ->
 * lc_attn_varlen_paged_bf16], capturable as one graph like its fp16 twin.  Each entry takes the arguments of its fp16 twin, one for one; every
 * 16-bit element — Q, O, Knew, Vnew, Qout and 16-bit pools — is read and written as bfloat16.  fp8 pools are the SAME OCP e4m3fn bytes under
 * the same fp32 per-head scales: a cache written by either element type is read by both.  cos_sin, sinks and the scales stay fp32.
 * The checks, their order and the statuses are the twin's: the same bad argument gets the same code.  So is the plan — RT, RB, S, the grid, the
 * LDS size and the workspace: lc_attn_varlen_paged_workspace_bytes / lc_attn_varlen_paged_kv8_workspace_bytes serve both element types (there
 * is no _bf16 workspace query), and "attn_decode_split" forces S as it does there.  The name calls report that plan with the kernels
 * attn_varlen_paged_bf16_kernel<D,RT> / attn_varlen_chunk_paged_bf16_kernel<D> / attn_varlen_paged_kv8_bf16_kernel<D,RT> /
 * attn_varlen_chunk_paged_kv8_bf16_kernel<D> (S > 1: + attn_varlen_combine_bf16_kernel<D>) and rope_append_varlen_bf16_kernel<D,INTERLEAVED> /
 * rope_append_varlen_kv8_bf16_kernel<D,INTERLEAVED>.
 * Arithmetic.  Attention: Q K^T and P V on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; P is rounded to bf16 (nearest even) while the
 * row sum keeps the unrounded fp32 value; the softmax state, the partials and their merge are fp32; O is rounded ONCE, fp32 -> bf16 nearest
 * even.  An fp8 cache is converted e4m3 -> bf16 in registers, exactly.  RoPE: bf16 -> fp32 (exact), the fp32 arithmetic of the fp16 entry,
 * ONE rounding to bf16 (nearest even, denormals kept); elements at or behind rot_dim and all of V are copied bit for bit; an fp8 pool gets
 * the code e4m3fn_rne(clamp(fp32(x) / scale, +-448)) of the rotated row ROUNDED TO bf16 FIRST (what a bf16 pool quantised afterwards would
 * hold), NaN -> a NaN code, +-inf -> +-448.
 * A ragged call whose Nq_b all equal max_nq is the rectangular call: the rectangular and contiguous-cache entries have no bf16 form.
 * Not here: bf16 forms of lc_attn_decode_* / lc_attn_chunk_* / lc_attn_local_* / lc_rope_append_paged_*, D outside {64, 128}, a 16-bit table. */
int lc_attn_varlen_paged_bf16(const void* Q, const void* Kpool, const void* Vpool, void* O,
                              const int* cu_q, const int* block_table, const int* kv_len,
                              int B, int H, int Hkv, int T, int max_nq,
                              int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                              void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                          int flags, char* buf, int buflen);
int lc_attn_varlen_paged_kv8_bf16(const void* Q, const void* Kpool8, const void* Vpool8, void* O,
                                  const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                                  int B, int H, int Hkv, int T, int max_nq,
                                  int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                  void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                              int flags, char* buf, int buflen);
int lc_rope_append_varlen_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                               const float* cos_sin, const int* cu_q, const int* block_table, const int* kv_len,
                               int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                               int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_kv8_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8,
                                   const float* cos_sin, const int* cu_q, const int* block_table, const int* kv_len,
                                   const float* k_scale, const float* v_scale,
                                   int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                                   int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                           int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                           char* buf, int buflen);
int lc_rope_append_varlen_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                               int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                               char* buf, int buflen);

/* EXTENSION: the ragged entries with a log-sum-exp output, and the merge of two attention states (attn_varlen_lse.hip, attn_merge.hip, DESIGN.md
 * section 4.3n) — what shared-prefix (cascade) attention, attention over KV shards and a windowed + global pass are built from.
 * lc_attn_varlen_paged_lse_f16 / _lse_kv8 / _lse_bf16 / _lse_kv8_bf16 take the arguments of lc_attn_varlen_paged_f16 / _kv8 / _bf16 /
 * _kv8_bf16 with `lse` right behind O:
 *   lse   device float32 [T H]: row t, head h at t H + h, the row of O.  lse = ln(sum over the row's visible keys of exp(score)), the sink of
 *         the head included; score = q.k / sqrt(D), times k_scale[head] for fp8 pools (v_scale does not enter).  A row that sees no key and
 *         has no sink: -inf (its O is 0).  Rows no sequence owns are written in neither buffer.
 * The checks, their order and the statuses are the twin's, with lse == NULL among the NULL pointers (LC_ERR_ARG).  So are the plan — RT, RB, S,
 * grid, LDS — and the workspace: lc_attn_varlen_paged_workspace_bytes / _kv8_workspace_bytes serve these entries too, and the capture / failed
 * lease fallback to S = 1 is the twin's.  O is the twin's O bit for bit.  The name calls report the twin's plan with "_lse" in the kernel:
 * attn_varlen_paged_lse_kernel<D,RT>, attn_varlen_chunk_paged_kv8_lse_bf16_kernel<D>, ... (S > 1: + attn_varlen_combine_lse_kernel<D> /
 * attn_varlen_combine_lse_bf16_kernel<D>).
 * lc_attn_merge_states_f16 / _bf16: (Oa, lse_a) and (Ob, lse_b) are the states of the SAME rows over two DISJOINT key sets, O [T,H,D] 16-bit,
 * lse float32 [T H]; the merged state is that of the union.  Per row in fp32: m = max(la, lb), wa = exp(la - m), wb = exp(lb - m),
 * O = (wa Oa + wb Ob) / (wa + wb) rounded once (nearest even), lse = m + ln(wa + wb).  One side -inf: the other passes through bit for bit.
 * Both -inf: O = 0, lse = -inf.  Oout may be Oa or Ob and lse_out may be lse_a or lse_b (in place).
 *   cu_q  NULL: all T H rows.  Else device int32 [B + 1], the offsets of the ragged calls: only the rows of tokens clamp(cu_q[0], 0, T) ..
 *         clamp(cu_q[B], 0, T) - 1 are read and written, so a captured step whose T is a bound keeps the rows behind its last token.
 * Status: a NULL pointer other than cu_q LC_ERR_ARG; B, T or H < 1, T H > 2^31 - 1 or an O pointer off 16 bytes LC_ERR_SHAPE; D outside
 * {64, 128} LC_ERR_HEADDIM.  attn_merge_states_kernel<D> / attn_merge_states_bf16_kernel<D>, no workspace.
 * Not here: an lse output of lc_attn_fwd_* and of the rectangular cache entries (a ragged call whose Nq_b all equal max_nq is the rectangular
 * call), an N-way merge in one launch, fp32 O partials between the levels. */
int lc_attn_varlen_paged_lse_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse,
                                 const int* cu_q, const int* block_table, const int* kv_len,
                                 int B, int H, int Hkv, int T, int max_nq,
                                 int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                 void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_lse_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                         int flags, char* buf, int buflen);
int lc_attn_varlen_paged_lse_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse,
                                 const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                                 int B, int H, int Hkv, int T, int max_nq,
                                 int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                 void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_lse_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                             int flags, char* buf, int buflen);
int lc_attn_varlen_paged_lse_bf16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse,
                                  const int* cu_q, const int* block_table, const int* kv_len,
                                  int B, int H, int Hkv, int T, int max_nq,
                                  int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                  void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_lse_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                              int flags, char* buf, int buflen);
int lc_attn_varlen_paged_lse_kv8_bf16(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse,
                                      const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                                      int B, int H, int Hkv, int T, int max_nq,
                                      int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                      void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_lse_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                                  int flags, char* buf, int buflen);
int lc_attn_merge_states_f16(const void* Oa, const float* lse_a, const void* Ob, const float* lse_b, void* Oout, float* lse_out,
                             const int* cu_q, int B, int T, int H, int D, void* stream);
int lc_attn_merge_states_bf16(const void* Oa, const float* lse_a, const void* Ob, const float* lse_b, void* Oout, float* lse_out,
                              const int* cu_q, int B, int T, int H, int D, void* stream);

/* EXTENSION: tree-structured speculative decoding on the ragged entries — a look-back visibility mask per query token, and per-token rotary
 * positions (attn_varlen_tree.hip, rope_append_varlen_pos.hip).  The new tokens of a sequence are the nodes of a draft
 * tree (Medusa, EAGLE, SpecInfer), appended to neighbouring cache slots: a node must see the prefix and its own ancestors, never its siblings,
 * and its rotary position is prefix length + depth, not its slot.
 * lc_attn_varlen_paged_tree_f16 / _tree_kv8 / _tree_bf16 / _tree_kv8_bf16 take the arguments of lc_attn_varlen_paged_lse_f16 / _lse_kv8 /
 * _lse_bf16 / _lse_kv8_bf16 with `tree_mask` right behind lse:
 *   tree_mask  device uint64 [T], 8-byte aligned: one word per token row of Q.  Token i of sequence b sits at cache slot p = L_b - Nq_b + i
 *         (the clamps of the ragged entries).  The twin's rule is unchanged: key j is visible iff j <= p, and iff j > p - W when a window is
 *         given.  The tree rule adds ONE condition: for d = p - j in [0, 64) the key is visible only if bit d of tree_mask[q0 + i] is set.
 *         Bit 0 is the token's own key.  Keys with d >= 64 are not governed by the mask.
 * A word of all ones is exactly the twin (same O and lse, bit for bit): an ordinary decoding or prefilling sequence of any Nq_b rides in the same
 * ragged batch with all-ones words.  A tree of up to 64 draft tokens is fully described: the ancestors of token i are at most i <= 63 slots
 * back.  A row whose mask hides every key behaves as "no visible key" does: O = 0 and lse = -inf, or the sink alone when sinks are given.
 * `window` keeps counting cache slots, not tree depth.
 * The checks, their order and the statuses are the twin's, with three additions: tree_mask == NULL among the NULL pointers (LC_ERR_ARG), a
 * tree_mask off 8 bytes among the misaligned pointers (LC_ERR_SHAPE), and a call without LC_ATTN_CAUSAL refused where a window without
 * LC_ATTN_CAUSAL is (LC_ERR_ARG).  The plan — RT, RB, S, grid, LDS — the workspace (lc_attn_varlen_paged_workspace_bytes / _kv8_workspace_bytes)
 * and the capture rules are the twin's: the mask only removes keys from the tiles the twin walks.  The name calls report the twin's plan with
 * "tree" in place of "lse": attn_varlen_paged_tree_kernel<D,RT>, attn_varlen_chunk_paged_kv8_tree_bf16_kernel<D>, ... (S > 1: + the twin's
 * attn_varlen_combine_lse_kernel<D> / attn_varlen_combine_lse_bf16_kernel<D>).
 * lc_rope_append_varlen_pos_f16 / _pos_kv8 / _pos_bf16 / _pos_kv8_bf16 take the arguments of lc_rope_append_varlen_f16 / _kv8 / _bf16 /
 * _kv8_bf16 with `pos_ids` right behind cu_q:
 *   pos_ids  device int32 [T]: the cos_sin row used for token t is clamp(pos_ids[t], 0, max_pos - 1).  Everything else is the twin's: the cache
 *         slot p = L_b - Nq_b + i the token is written to, the p < 0 rule, dropped tokens, quantisation, strides and in-place Q.
 *         pos_ids[t] = p for every token gives the twin's bytes.  pos_ids == NULL: LC_ERR_ARG.
 * rope_append_varlen_pos_kernel<D,INTERLEAVED>, _pos_kv8_kernel, _pos_bf16_kernel, _pos_kv8_bf16_kernel.
 * Not here: trees of more than 64 tokens; masks on the rectangular, contiguous-cache or lc_attn_fwd_* entries; tree forms without lse; a tree
 * mask inside a cascade's prefix pass; compacting the accepted path's K / V after verification; M-RoPE (several position streams); a window
 * counted in tree depth. */
int lc_attn_varlen_paged_tree_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const uint64_t* tree_mask,
                                  const int* cu_q, const int* block_table, const int* kv_len,
                                  int B, int H, int Hkv, int T, int max_nq,
                                  int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                  void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_tree_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                          int flags, char* buf, int buflen);
int lc_attn_varlen_paged_tree_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse, const uint64_t* tree_mask,
                                  const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                                  int B, int H, int Hkv, int T, int max_nq,
                                  int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                  void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_tree_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                              int flags, char* buf, int buflen);
int lc_attn_varlen_paged_tree_bf16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const uint64_t* tree_mask,
                                   const int* cu_q, const int* block_table, const int* kv_len,
                                   int B, int H, int Hkv, int T, int max_nq,
                                   int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                   void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_tree_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                               int flags, char* buf, int buflen);
int lc_attn_varlen_paged_tree_kv8_bf16(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse, const uint64_t* tree_mask,
                                       const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                                       int B, int H, int Hkv, int T, int max_nq,
                                       int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                                       void* workspace, size_t workspace_bytes, void* stream);
int lc_attn_varlen_paged_tree_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window,
                                                   int flags, char* buf, int buflen);
int lc_rope_append_varlen_pos_f16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                  const float* cos_sin, const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len,
                                  int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                                  int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_pos_kv8(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8,
                                  const float* cos_sin, const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len,
                                  const float* k_scale, const float* v_scale,
                                  int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                                  int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_pos_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                                   const float* cos_sin, const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len,
                                   int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                                   int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_pos_kv8_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8,
                                       const float* cos_sin, const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len,
                                       const float* k_scale, const float* v_scale,
                                       int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                                       int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream);
int lc_rope_append_varlen_pos_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                          int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                          char* buf, int buflen);
int lc_rope_append_varlen_pos_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                              int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                              char* buf, int buflen);
int lc_rope_append_varlen_pos_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                               int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                               char* buf, int buflen);
int lc_rope_append_varlen_pos_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D,
                                                   int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                                                   char* buf, int buflen);

/* EXTENSION (BASELINE config 5 "FFPA-style QKV fine-grained tiling D=512 bf16"; the reference has no bf16
 * entry): the large-head-dim d-slice tiling kernel on bfloat16 Q,K,V,O [B,H,N,D], D in {256, 512}. */
int lc_attn_fwd_bf16(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                     void* stream);

/* Dispatch by the reference's export name (flash_attn.cc:170-223). */
int lc_attn_call(const char* entry, const void* Q, const void* K, const void* V, void* O, int B, int H,
                 int N, int D, int stages, void* stream);
int lc_attn_entry_count(void);
const char* lc_attn_entry_name(int index);
/* family (lc_attn_family), v_transposed, acc_f32, max head dim for stages>1 / stages<=1 and number of
 * reference arguments (4 for flash_attn_cute, else 5). */
int lc_attn_entry_info(const char* entry, int* family, int* v_transposed, int* acc_f32,
                       int* max_d_stage2, int* max_d_stage1, int* nargs);

/* ---- introspection (bench.py labels its roofline / rocprof rows with these; never launches) ------
 * Name of the kernel the dispatcher would launch for this call with the current lc_tune_set selection, in the form
 * rocprofv3 demangles it to (e.g. "hgemm_w4b_kernel<false,true,false,0>"), written NUL-terminated into buf.
 * Pointers are assumed 16-byte aligned.  Returns LC_OK, LC_ERR_ARG / LC_ERR_SHAPE / LC_ERR_HEADDIM as the call would. */
int lc_hgemm_kernel_name(int M, int N, int K, int layout, int variant, char* buf, int buflen);
int lc_attn_kernel_name(int N, int D, int v_transposed, int bf16, char* buf, int buflen);
/* the same for a launch of BH = batch x heads problems: where the choice depends on how far the grid fills the GPU (D = 256, "attn_d512"
 * above) the name is the kernel THAT launch runs; BH <= 0 = lc_attn_kernel_name (a grid that fills the GPU) */
int lc_attn_kernel_name_bh(int BH, int N, int D, int v_transposed, int bf16, char* buf, int buflen);
/* the kernel lc_attn_fwd_f16_ex runs for these flags (never launches; without LC_ATTN_CAUSAL: lc_attn_kernel_name_bh's answer) */
int lc_attn_kernel_name_ex(int BH, int N, int D, int flags, char* buf, int buflen);
/* How often the overflow slow path of the merged-phase attention kernels (attn_w4u.hip, attn_w4i.hip) ran since the last reset:
 * out4 = { executions, sum of their KV half-tile indices, executions that saw a non-finite row sum, bit pattern (fp32) of the
 * last offending row sum }.  Synchronises the device (hipMemcpyFromSymbol).  out4 may be NULL (reset only). */
int lc_attn_slowpath_stats(unsigned* out4, int reset);

/* ---- measurement helpers (used by bench.py; HIP events on the launch stream) --------------------
 * Launch `iters` back-to-back calls between two hipEvents recorded on `stream`; returns average
 * milliseconds per launch in *ms_per_launch.  Any HIP failure (event, launch, execution fault) -> LC_ERR_LAUNCH. */
int lc_hgemm_time(const void* A, const void* B, void* C, int M, int N, int K, int layout, int variant,
                  int stages, int swizzle_stride, int warmup, int iters, void* stream,
                  float* ms_per_launch);
int lc_attn_time(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                 int v_transposed, int family, int stages, int warmup, int iters, void* stream,
                 float* ms_per_launch);
/* Generic form: bracket ANY sequence of launches on `stream` with HIP events.  lc_timer_start records the first
 * event and returns an opaque timer; lc_timer_stop records the second, waits for it, writes the elapsed
 * milliseconds and frees the timer (also on failure). */
int lc_timer_start(void* stream, void** timer);
int lc_timer_stop(void* timer, float* elapsed_ms);
/* Effective shader clock without a profiler: a one-wave kernel writes {s_memtime (shader cycles), s_memrealtime
 * (constant 100 MHz)} into out_u64x2 (device memory).  Two probes around a timed batch on the same stream give
 * eff_clock = d(memtime) / (d(memrealtime) / 100e6). */
int lc_clock_probe(void* out_u64x2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LC_ABI_H_ */
