// tu_plan.hip — host-only translation unit: the tuning knobs, the reference entry-name tables and the launch planners — see lc_plan.h
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "lc_plan.h"

namespace lc {

// the knobs: storage and default (lc_knobs.inc)
#define LC_KNOB(name, dflt, valid, diag) tune_t g_tune_##name{dflt};
#include "lc_knobs.inc"

Knobs read_knobs() {
  Knobs k;
#define LC_KNOB(name, dflt, valid, diag)
#define LC_KNOB_SNAP(name, dflt, valid, diag) k.name = g_tune_##name;
#include "lc_knobs.inc"
  return k;
}

// the knob registry: the validators, and one row of kKnobs per row of lc_knobs.inc
namespace {
bool ok_attn_nw(int v) {
  return v == 0 || v == 512 || v == 513 || v == 514 || v == 515 || v == 517 || v == 8 || v == 4 || v == 2;
}
bool ok_01(int v) { return v == 0 || v == 1; }
bool ok_02(int v) { return v >= 0 && v <= 2; }
bool ok_03(int v) { return v >= 0 && v <= 3; }
bool ok_04(int v) { return v >= 0 && v <= 4; }
bool ok_08(int v) { return v >= 0 && v <= 8; }
bool ok_064(int v) { return v >= 0 && v <= 64; }
bool ok_rule_cus(int v) { return v == 0 || (v >= 64 && v <= 1024); }
bool ok_mid_ns(int v) { return v == 0 || v == 2 || v == 3; }
bool ok_ragged_tile(int v) { return v == 0 || v == 12 || v == 22 || v == 23 || v == 32 || v == 33; }
bool ok_mid(int v) { return v == 0 || v == 1 || v == 12 || v == 13 || v == 22 || v == 23 || v == 32 || v == 33; }
bool ok_split(int v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8 || v == 16; }
bool ok_span8(int v) { return v == 0 || v == 2 || v == 4 || v == 6; }
bool ok_w4y_sched(int v) {
#ifdef LC_DIAG
  return v >= 0 && v <= 6;   // 3..5: ablations (results WRONG); 6: the pair loop's k-step-outer twin (hgemm_w4y_loop2.inc)
#else
  return v >= 0 && v <= 2;
#endif
}
// cx | cm << 4 | cn << 8 | step << 12 | mask << 20 with a 7-bit mask (bits 20 .. 26), or exactly STAGGER_OFF (1 << 27)
bool ok_stagger(int v) { return v >= 0 && ((v >> 27) == 0 || v == STAGGER_OFF); }
bool ok_auto(int v) { return is_tile256_variant(v); }
bool ok_any(int) { return true; }
}  // namespace
const Knob kKnobs[] = {
#define LC_KNOB(name, dflt, valid, diag) {#name, &g_tune_##name, dflt, valid, diag},
#include "lc_knobs.inc"
};
const int kNumKnobs = (int)(sizeof(kKnobs) / sizeof(kKnobs[0]));
const Knob* find_knob(const char* key) {
  if (!key) return nullptr;
  for (const Knob& k : kKnobs)
    if (strcmp(k.key, key) == 0) {
#ifndef LC_DIAG
      if (k.diag) return nullptr;
#endif
      return &k;
    }
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// reference entry tables
#define NN LC_LAYOUT_NN
#define TN LC_LAYOUT_TN
// kernels/hgemm/pybind/hgemm.cc:126-181, in the reference's registration order.
const HgemmEntry kHgemmEntries[] = {
    {"hgemm_naive_f16", NN, 3, LC_HGEMM_VALU_NAIVE},
    {"hgemm_sliced_k_f16", NN, 3, LC_HGEMM_VALU_SLICED_K},
    {"hgemm_t_8x8_sliced_k_f16x4", NN, 3, LC_HGEMM_VALU_T8X8_X4},
    {"hgemm_t_8x8_sliced_k_f16x4_pack", NN, 3, LC_HGEMM_VALU_T8X8_X4_PACK},
    {"hgemm_t_8x8_sliced_k_f16x4_bcf", NN, 3, LC_HGEMM_VALU_T8X8_X4_BCF},
    {"hgemm_t_8x8_sliced_k_f16x4_pack_bcf", NN, 3, LC_HGEMM_VALU_T8X8_X4_PACK_BCF},
    {"hgemm_t_8x8_sliced_k_f16x8_pack_bcf", NN, 3, LC_HGEMM_VALU_T8X8_X8_PACK_BCF},
    {"hgemm_t_8x8_sliced_k_f16x8_pack_bcf_dbuf", NN, 3, LC_HGEMM_VALU_T8X8_X8_PACK_BCF_DBUF},
    {"hgemm_t_8x8_sliced_k16_f16x8_pack_dbuf", NN, 3, LC_HGEMM_VALU_T8X8_K16},
    {"hgemm_t_8x8_sliced_k16_f16x8_pack_dbuf_async", NN, 3, LC_HGEMM_VALU_T8X8_K16},
    {"hgemm_t_8x8_sliced_k32_f16x8_pack_dbuf", NN, 3, LC_HGEMM_VALU_T8X8_K32},
    {"hgemm_t_8x8_sliced_k32_f16x8_pack_dbuf_async", NN, 3, LC_HGEMM_VALU_T8X8_K32},
    {"hgemm_t_16x8_sliced_k32_f16x8_pack_dbuf", NN, 3, LC_HGEMM_VALU_T16X8_K32},
    {"hgemm_t_16x8_sliced_k32_f16x8_pack_dbuf_async", NN, 3, LC_HGEMM_VALU_T16X8_K32},
    {"init_cublas_handle", NN, 0, -2},
    {"destroy_cublas_handle", NN, 0, -3},
    {"hgemm_cublas_tensor_op_nn", NN, 3, -1},
    {"hgemm_cublas_tensor_op_tn", TN, 3, -1},
    {"hgemm_wmma_m16n16k16_naive", NN, 3, LC_HGEMM_GENERIC},
    {"hgemm_wmma_m16n16k16_mma4x2", NN, 3, LC_HGEMM_GENERIC},
    {"hgemm_wmma_m16n16k16_mma4x2_warp2x4", NN, 3, LC_HGEMM_MFMA128},
    {"hgemm_wmma_m16n16k16_mma4x2_warp2x4_dbuf_async", NN, 3, LC_HGEMM_MFMA128},
    {"hgemm_wmma_m32n8k16_mma2x4_warp2x4_dbuf_async", NN, 3, LC_HGEMM_MFMA128},
    {"hgemm_wmma_m16n16k16_mma4x2_warp2x4_stages", NN, 6, LC_HGEMM_MFMA256},
    {"hgemm_wmma_m16n16k16_mma4x2_warp2x4_stages_dsmem", NN, 6, LC_HGEMM_MFMA256},
    {"hgemm_wmma_m16n16k16_mma4x2_warp4x4_stages_dsmem", NN, 6, LC_HGEMM_MFMA256P2},
    {"hgemm_wmma_m16n16k16_mma4x4_warp4x4_stages_dsmem", NN, 6, LC_HGEMM_MFMA256P2},
    {"hgemm_mma_m16n8k16_naive", NN, 3, LC_HGEMM_GENERIC},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4", NN, 3, LC_HGEMM_MFMA256},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4_stages", NN, 6, LC_HGEMM_MFMA256},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4_stages_dsmem", NN, 6, LC_HGEMM_MFMA256},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem", NN, 6, LC_HGEMM_AUTO},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem_x4", NN, 6, LC_HGEMM_AUTO},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem_rr", NN, 6, LC_HGEMM_AUTO},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem_swizzle", NN, 6, LC_HGEMM_AUTO},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4_stages_dsmem_tn", TN, 6, LC_HGEMM_MFMA256},
    {"hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem_tn_swizzle_x4", TN, 6, LC_HGEMM_AUTO},
    {"hgemm_mma_stages_block_swizzle_tn_cute", TN, 6, LC_HGEMM_AUTO},
};
#undef NN
#undef TN
const int kNumHgemmEntries = sizeof(kHgemmEntries) / sizeof(kHgemmEntries[0]);

// kernels/flash-attn/pybind/flash_attn.cc:170-223; head-dim limits from each wrapper's switch(d)
// (e.g. flash_attn_mma_split_q.cu:769-815, flash_attn_mma_share_qkv.cu:872-921).
const AttnEntry kAttnEntries[] = {
    {"flash_attn_mma_stages_split_kv", LC_ATTN_SPLIT_KV, 0, 0, 128, 128, 5},
    {"flash_attn_mma_stages_split_q", LC_ATTN_SPLIT_Q, 0, 0, 128, 128, 5},
    {"flash_attn_mma_stages_split_q_shared_kv", LC_ATTN_SHARED_KV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_qkv", LC_ATTN_SHARED_QKV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_tiling_qk", LC_ATTN_TILING_QK, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv", LC_ATTN_TILING_QKV, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_shared_kv_acc_f32", LC_ATTN_SHARED_KV, 0, 1, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_qkv_acc_f32", LC_ATTN_SHARED_QKV, 0, 1, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_tiling_qk_acc_f32", LC_ATTN_TILING_QK, 0, 1, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_acc_f32", LC_ATTN_TILING_QKV, 0, 1, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_shared_kv_swizzle_q", LC_ATTN_SHARED_KV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_kv_swizzle_qk", LC_ATTN_SHARED_KV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_kv_swizzle_qkv", LC_ATTN_SHARED_KV, 1, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_qkv_swizzle_q", LC_ATTN_SHARED_QKV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_qkv_swizzle_qk", LC_ATTN_SHARED_QKV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_qkv_swizzle_qkv", LC_ATTN_SHARED_QKV, 1, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_tiling_qk_swizzle_q", LC_ATTN_TILING_QK, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qk_swizzle_qk", LC_ATTN_TILING_QK, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qk_swizzle_qkv", LC_ATTN_TILING_QK, 1, 0, 256, 256, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_swizzle_q", LC_ATTN_TILING_QKV, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_swizzle_qk", LC_ATTN_TILING_QKV, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_swizzle_qkv", LC_ATTN_TILING_QKV, 0, 0, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_acc_f32_swizzle_q", LC_ATTN_TILING_QKV, 0, 1, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_acc_f32_swizzle_qk", LC_ATTN_TILING_QKV, 0, 1, 1024, 1024, 5},
    {"flash_attn_mma_stages_split_q_tiling_qkv_acc_f32_swizzle_qkv", LC_ATTN_TILING_QKV, 0, 1, 1024, 1024, 5},
    {"flash_attn_cute", LC_ATTN_SPLIT_Q, 0, 1, 256, 256, 4},
    // -DBUILD_FLASH_ATTN_MMA_OTHERS (flash_attn.cc:217-223)
    {"flash_attn_mma_stages_split_q_shared_qkv_Os2g", LC_ATTN_SHARED_QKV, 0, 0, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_kv_acc_f32_rr", LC_ATTN_SHARED_KV, 0, 1, 128, 256, 5},
    {"flash_attn_mma_stages_split_q_shared_qkv_acc_f32_rr", LC_ATTN_SHARED_QKV, 0, 1, 256, 256, 5},
};
const int kNumAttnEntries = sizeof(kAttnEntries) / sizeof(kAttnEntries[0]);

const HgemmEntry* find_hgemm(const char* name) {
  if (!name) return nullptr;
  for (int i = 0; i < kNumHgemmEntries; ++i)
    if (strcmp(kHgemmEntries[i].name, name) == 0) return &kHgemmEntries[i];
  return nullptr;
}
const AttnEntry* find_attn(const char* name) {
  if (!name) return nullptr;
  for (int i = 0; i < kNumAttnEntries; ++i)
    if (strcmp(kAttnEntries[i].name, name) == 0) return &kAttnEntries[i];
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// kernel selection: the rules (each reads the knob snapshot it is given, never a global)
bool is_w4_variant(int v) {
  return v == LC_HGEMM_MFMA256W4B || v == LC_HGEMM_MFMA256W4C || v == LC_HGEMM_MFMA256W4X ||
         v == LC_HGEMM_MFMA256W4Y;
}
bool is_tile256_variant(int v) { return v == LC_HGEMM_MFMA256 || v == LC_HGEMM_MFMA256P2 || is_w4_variant(v); }
bool is_valu_variant(int v) { return v >= LC_HGEMM_VALU_NAIVE && v <= LC_HGEMM_VALU_T16X8_K32; }
bool is_hgemm_variant(int v) {
  return v == LC_HGEMM_AUTO || v == LC_HGEMM_GENERIC || v == LC_HGEMM_EDGE || v == LC_HGEMM_RAGGED || v == LC_HGEMM_KPAD || v == LC_HGEMM_MFMA128 || v == LC_HGEMM_MID || is_tile256_variant(v) || is_valu_variant(v);
}

// Block -> C tile map handed to the tiled kernels (block_tile, hgemm_mfma256.hip): >= 1 = the reference's block swizzle with
// that many tile columns per N panel, -1 = XCD super-block raster.  Auto rule (measured, profiles/r3b_hgemm_raster_ab.log,
// 0.5 s sustained per cell, 3 interleaved rounds): operands that fit the 256 MiB Infinity Cache are served from it whatever
// the order (8192^3: A + B = 256 MiB, block swizzle 1441 / xcd16 1435 TFLOP/s TN; 4096^3 +0.2 %), beyond it the super-block
// raster streams every panel from HBM about a third as often: 12544^3 +5.7 %, 15360^3 +8.3 %, 16384^3 +5.3 % TN (+4.7 ... 6.9 %
// NN), which is what lifts AUTO from 4 ... 9 % behind hipBLASLt TN to level with it on the reference's published sizes.
int panel_tiles(int raster, int swizzle_stride, int tiles_n, int tile_n, size_t operand_bytes) {
  // (round 6: the threshold came down from 1.5 x to 1.0625 x the Infinity Cache — 8704^3 + 3.2 %, 8960^3 + 4.2 %, 9728^3 + 4.3 % with the super-block
  // raster, 9216^3 level, 8192^3 and below 0.3 ... 1.3 % better on the block swizzle: profiles/r6i_hgemm_knob_sched_ab.log)
  const bool xcd16 = raster == 2 || (raster == 0 && operand_bytes > ((size_t)272 << 20));
  if (xcd16) return -1;                     // the kernel ignores the stride
  if (swizzle_stride <= 1) return tiles_n;  // no thread-block swizzle: plain N-major raster
  int w = swizzle_stride / tile_n;
  if (w < 1) w = 1;
  if (w > tiles_n) w = tiles_n;
  return w;
}

// The CU count the launch rules reason with (lc_tune_set "rule_cus"): the device's own unless a test asks what a 128- or 304-CU part would
// be told.  Only RULES use it (which kernel, which tile, which split factor); every grid is sized with device_cu_count().
int rule_cus(const Knobs& k) { return k.rule_cus > 0 ? k.rule_cus : device_cu_count(); }
AttnCalib g_attn_calib[64];

namespace {
// Waves of hgemm_mfma128_kernel for a launch of `blocks` 128 x 128 tiles (lc_tune_set "hgemm_128w"): eight (KSW = 2, two waves per SIMD
// inside one block) on grids that leave CUs idle, four otherwise.  Measured (profiles/r5g_hgemm_128w.log, four vs eight waves, TN / NN):
// 1024^3 (64 blocks) 172 / 167 -> 192 / 189 TFLOP/s, 1536^3 (144) 410 / 396 -> 454 / 425; 2048^3 (256 blocks = one per CU) 705 -> 701: level —
// there the 128 x 128 tile is bound by L2 bandwidth (64 FLOP / B: 10 TB/s at 700 TFLOP/s), not by latency, and from 2560^3 on the NN form
// LOSES (825 -> 587: twice the waves on the transpose reads).  Auto: eight up to 0.6 blocks per CU.
int mfma128_ksw(const Knobs& k, long blocks) {
  if (k.hgemm_128w == 1 || k.hgemm_128w == 2) return k.hgemm_128w;
  return 5 * blocks <= 3 * (long)rule_cus(k) ? 2 : 1;
}

// The mid-size kernel (hgemm_mid.hip; lc_tune_set "hgemm_mid", "hgemm_mid_ns"): which tile serves this shape, tmw == 0 = not this kernel.
// Auto = hipBLASLt's own heuristic for these sizes read off its kernel names (profiles/r6a_vendor_kernels.log) and measured here tile by
// tile (profiles/r6c_hgemm_mid_ab.log): when a tile's grid fits ONE ROUND of at most one workgroup per CU, the smallest such tile — most
// workgroups, least work on the busiest CU — with three ring slots (the DMA two tiles ahead): 64 x 128 at 1024 / 1280, 64 x 192 at 1536
// TN, 128 x 128 at 1536 NN / 1792 / 2048, 128 x 192 at 2304 TN, 192 x 128 at 2304 NN (the 64-row tiles lose to the 128-row ones as soon as both need more than a
// round: 2304 NN 780 vs 866 TFLOP/s, 2560 646 vs 983); otherwise 128 x 128 with two slots and two workgroups per CU (2304 NN, 2560, 2816).
// `gated` (LC_HGEMM_AUTO): only where the 256-tile kernel does not apply anyway (plan_hgemm: <= 128 tiles of 256 x 256) and the
// 128 x 128 grid holds more than 3 / 16 blocks per CU (below — 768^3: 36 blocks, level — the eight-wave 128-tile kernel keeps the shape).
MidTile mid_tile_auto(const Knobs& kn, int M, int N, int K, bool b_kn, bool gated) {
  MidTile none{0, 0, 0, 1, 0};
  if (M % 64 != 0 || N % 64 != 0 || K % 32 != 0 || K < BK || K >= (1 << 22) || N >= (1 << 22)) return none;
  const int k = kn.hgemm_mid, kns = kn.hgemm_mid_ns;
  if (k == 1 && gated) return none;
  const long ncu = rule_cus(kn);
  const long min_blocks = 3 * ncu / 16;   // 48 of 128 x 128 on 256 CUs (768^3: 36 blocks, level with the eight-wave kernel; 1024^3: 64 blocks, + 15 %)
  // (... unless K is long enough to split: 512 x 512 x 8192 runs 32 workgroups x 8 K ranges here)
  const bool long_k = kn.hgemm_mid_splitk != 1 && K / BK >= 64;   // (two ranges of 32 K tiles)
  // (M or N a multiple of 64 only — 2880^3 — has no other tiled kernel: any tile that divides it beats hgemm_generic_kernel by 10 x)
  if (gated && M % 128 == 0 && N % 128 == 0 && (long)(M / 128) * (N / 128) <= min_blocks && !long_k) return none;
  MidTile best = none, big = none;
  long best_wgs = 0;   // best one-round tile; largest legal tile (the multi-round choice)
  long best_area = 0, big_area = 0;
  for (int tmw : {2, 3, 1})        // (ties between equal areas go to the tile seen first: 128 x 192 before 192 x 128)
    for (int tnw = 2; tnw <= 3; ++tnw) {
      if (k >= 10 && k != 10 * tmw + tnw) continue;
      if (M % (64 * tmw) != 0 || N % (64 * tnw) != 0 || (b_kn && tnw != 2)) continue;
      const long wgs = (long)(M / (64 * tmw)) * (N / (64 * tnw)), area = 4096L * tmw * tnw;
      if (wgs <= ncu && (best.tmw == 0 || area < best_area)) {
        best = MidTile{tmw, tnw, 3, 1, wgs};
        best_area = area;
        best_wgs = wgs;
      }
      // multi-round: 128 x 128 before 128 x 192 (one workgroup per CU by registers) before the 64-row tiles
      const long rank = (tmw == 2 && tnw == 2) ? 5 : (tmw == 2 ? 4 : tmw == 3 ? 3 : tnw - 1);
      if (big.tmw == 0 || rank > big_area) {
        big = MidTile{tmw, tnw, 2, 1, 0};
        big_area = rank;
      }
    }
  // 192 x 192 is the one tile with more work per CU (36864 outputs) than a double round of 128 x 128 at two workgroups per CU (2 x 16384):
  // it wins only where the 128 x 128 grid needs more than one such round (3072^3: 576 blocks; 3072 x 2304: 432 blocks, 950 vs 1016 TFLOP/s)
  if (best.tmw && best_area > 32768 && k < 10 && big.tmw == 2 && big.tnw == 2 && (long)(M / 128) * (N / 128) <= 2 * ncu) best = none;
  MidTile t = best.tmw ? best : big;
  if (!best.tmw && t.tmw * t.tnw >= 6) t.ns = 3;   // one workgroup per CU by registers anyway: the third slot is free (8192 x 8256 x 4096 TN: 1004 -> 1108)
  if (t.tmw && (kns == 2 || kns == 3)) t.ns = kns;
  // split-K (round 6, lc_tune_set "hgemm_mid_splitk"): a one-round grid on at most half the CUs with a long K — as many K ranges as fill
  // the CUs, each of at least 32 K tiles (1024 x 1024 x 8192: 128 workgroups x 2, 512 -> 620 TFLOP/s; 1024 x 1024 x 2048 with 16 tiles per range: 415 -> 306;
  // profiles/r6p_hgemm_rect_splitk.log); never at the reference sweep's sizes (1024^3: 16 K tiles)
  const int ksk = kn.hgemm_mid_splitk, KT = K / BK;
  if (best.tmw && t.tnw == 2 && t.tmw <= 2 && ksk != 1) {
    long ks = ksk >= 2 ? ksk : std::min<long>(std::min<long>(ncu / best_wgs, KT / 32), 8);
    while (ks > 1 && KT < 2 * ks) --ks;
    if (ks > 1 && (size_t)ks * M * N * sizeof(float) <= ((size_t)256 << 20)) {
      t.ks = (int)ks;
      t.ns = 3;
    }
  }
  return t;
}

// LC_HGEMM_KPAD (late round 6): K is not a multiple of 32 (K % 8 == 0, N % 8 == 0) on a problem large enough that hgemm_edge_kernel's 0.5 ... 0.66 x of the
// vendor hurts: A and B are copied into this stream's workspace with K padded to the next multiple of 32 by zeros (products with zero add nothing to an
// fp32 sum: the result is what the tuned kernels would produce on the padded problem, exactly), and the padded problem runs LC_HGEMM_AUTO's choice —
// tiled or LC_HGEMM_RAGGED, in its workspace-free form (the operands hold the workspace).  Costs two copies (8192 x 8192 x 8200: 0.54 GB of traffic).
// Not under graph capture, not beyond the workspace cap: the edge kernel then.  Kp = 0: not this path.
int kpad_plan(const Knobs& k, int M, int N, int K, bool al, bool gated) {
  if (!al || K % 8 != 0 || K % 32 == 0 || N % 8 != 0 || K < 256 || K >= (1 << 22) - 32 || N >= (1 << 22)) return 0;
  const int knob = k.hgemm_kpad;
  if (gated && knob == 1) return 0;
  const long eb = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (gated && knob == 0 && 4 * eb < rule_cus(k)) return 0;   // (below a quarter of a block per CU three launches cost more than the edge kernel's slower K walk; 1000^3: + 20 %, 8192 x 8192 x 8200: + 75 %)
  const int Kp = (K + 31) / 32 * 32;
  if (((size_t)M + N) * Kp * 2 > kWorkspaceCapBytes) return 0;
  return Kp;
}

// buffer-descriptor DMA addresses are 32-bit offsets from the wave's first row: fall back to the 64-bit global form
// when an offset could reach 2 GiB (NN: K tiles step through the whole of B)
int w4_effective_variant(int variant, bool b_kn, int N, int K) {
  if (variant == LC_HGEMM_MFMA256W4X && b_kn) variant = LC_HGEMM_MFMA256W4C;   // the compiler-scheduled 16x16x32 kernel is TN only
  if (variant == LC_HGEMM_MFMA256W4C || variant == LC_HGEMM_MFMA256W4X ||
      variant == LC_HGEMM_MFMA256W4Y) {
    // (K-contiguous operands: a wave's pieces reach 64 rows past its base, 232 with hgemm_w4y's 32-row piece stride: w4_rows_fit)
    const bool rows_fit = variant == LC_HGEMM_MFMA256W4Y ? w4_rows_fit(K, 2) : (size_t)K * 2 * 130 < ((size_t)1 << 31);
    if (!rows_fit || (b_kn && (size_t)K * N * 2 + (size_t)N * 64 >= ((size_t)1 << 31))) return LC_HGEMM_MFMA256W4B;
  }
  return variant;
}

// LC_HGEMM_RAGGED (late round 6): M and / or N are not multiples of the tiles (not legal in the reference, hgemm_mma_stage.cu:675-676), K is
// (K % 32 == 0, K >= 64) and rows are 16-byte aligned (N % 8 == 0).  The tiled kernels take N as C's / B's row stride and their tile counts
// separately, and hgemm_mid_edge_kernel (hgemm_mid.hip EDGE) runs 128 x 128 tiles that reach beyond M / N (clamped sources, predicated stores):
//   kind 1  more than half a CU's worth of 256 x 256 tiles: the INTERIOR — the largest top-left sub-matrix they divide — on hgemm_w4y_kernel exactly
//           as a problem of its own (+ its ragged last round on the mid-size kernel, tail_split), the L-shaped BORDER (right strip: all rows x
//           columns Ni .. N, bottom strip: rows Mi .. M x columns 0 .. Ni) on hgemm_mid_edge_kernel in a second launch
//   kind 2  otherwise: the whole problem on hgemm_mid_edge_kernel (three ring slots while the tiles fit one round of the CUs, else two)
// Every element of C is computed by exactly one kernel, deterministically; no workspace.  lc_tune_set "hgemm_ragged" = 1: never (hgemm_edge_kernel).
RaggedPlan ragged_plan(const Knobs& k, int M, int N, int K, bool al, bool b_kn, bool gated) {
  RaggedPlan none{0, 0, 0, 0, 0, 0, 1};
  if (!al || K % 32 != 0 || K < BK || N % 8 != 0 || K >= (1 << 22) || N >= (1 << 22)) return none;
  if (M % BM1 == 0 && N % BN1 == 0) return none;   // (a tiled shape)
  if (gated && k.hgemm_ragged == 1) return none;
  const long ncu = rule_cus(k);
  const long t256 = (long)(M / BM) * (N / BN);
  if (2 * t256 > ncu && k.hgemm_auto == LC_HGEMM_MFMA256W4Y && w4_effective_variant(LC_HGEMM_MFMA256W4Y, b_kn, N, K) == LC_HGEMM_MFMA256W4Y) {
    const int Mi = (M / BM) * BM, Ni = (N / BN) * BN;
    const long nb = (long)((N - Ni + 127) / 128) * ((M + 127) / 128) + (long)((M - Mi + 127) / 128) * (Ni / 128);   // border blocks
    return RaggedPlan{1, Mi, Ni, nb <= ncu ? 3 : 2, 2, 2, 1};
  }
  // the mid-size kernel's own rule (mid_tile_auto; measured on ragged shapes in profiles/r6ag_hgemm_edge_ab.log): the smallest tile whose grid fits ONE round of
  // at most one workgroup per CU (most workgroups, least work on the busiest CU; three ring slots) — 64 x 128, 128 x 128, then 128 x 192 (TN) / 192 x 128 (NN:
  // 128-column tiles only); where 128 x 128 at two per CU needs more than one double round, 192 x 192 (TN; 3000 x 3000 x 3008: 1074 vs 783 TFLOP/s) /
  // 192 x 128 (NN: 865 vs 724); else 128 x 128 with two slots at two workgroups per CU (2500 x 2504 x 2560 TN: 857 vs 773 on 192 x 192 in one round).
  const int tile_knob = k.hgemm_ragged_tile;
  // split-K as the mid-size kernel's own (mid_tile_auto, "hgemm_mid_splitk"): a one-round grid of 64 / 128 x 128 tiles on at most half the CUs with a long K — as
  // many K ranges as fill the CUs, each of at least 32 K tiles, at most 8 (100 x 4096 x 4096: 64 workgroups x 2)
  auto split_k = [&](RaggedPlan p) {
    const int ksk = k.hgemm_mid_splitk, KT = K / BK;
    const long wgs = (long)((M + 64 * p.tmw - 1) / (64 * p.tmw)) * ((N + 127) / 128);
    if (p.tnw != 2 || p.tmw > 2 || p.ns != 3 || ksk == 1 || wgs > ncu) return p;
    long ks = ksk >= 2 ? ksk : std::min<long>(std::min<long>(ncu / wgs, KT / 32), 8);
    while (ks > 1 && KT < 2 * ks) --ks;
    if (ks > 1 && launch_hgemm_mid_edge_sk_floats(M, N, p.tmw, (int)ks) * sizeof(float) <= ((size_t)256 << 20)) p.ks = (int)ks;
    return p;
  };
  auto blocks_of = [&](int tmw, int tnw) { return (long)((M + 64 * tmw - 1) / (64 * tmw)) * ((N + 64 * tnw - 1) / (64 * tnw)); };
  if (tile_knob != 0) {
    const int tmw = tile_knob / 10, tnw = tile_knob % 10;
    const bool legal = b_kn ? tnw == 2 : !(tmw == 3 && tnw == 2);
    if (legal) return split_k(RaggedPlan{2, 0, 0, (tmw == 2 && tnw == 2 && blocks_of(2, 2) > ncu) ? 2 : 3, tmw, tnw, 1});
  }
  if (blocks_of(1, 2) <= ncu) return split_k(RaggedPlan{2, 0, 0, 3, 1, 2, 1});
  if (blocks_of(2, 2) <= ncu) return split_k(RaggedPlan{2, 0, 0, 3, 2, 2, 1});
  if (blocks_of(2, 2) > 2 * ncu) return b_kn ? RaggedPlan{2, 0, 0, 3, 3, 2, 1} : RaggedPlan{2, 0, 0, 3, 3, 3, 1};
  if (b_kn ? blocks_of(3, 2) <= ncu : blocks_of(2, 3) <= ncu) return b_kn ? RaggedPlan{2, 0, 0, 3, 3, 2, 1} : RaggedPlan{2, 0, 0, 3, 2, 3, 1};
  return RaggedPlan{2, 0, 0, 2, 2, 2, 1};
}

// Ragged last round of hgemm_w4y_kernel (lc_tune_set "hgemm_tail" = `knob`): T tiles on ncu CUs run ceil(T / ncu) tile periods, the last one
// with R = T % ncu workgroups (the device's own CU count, the figure the persistent launchers use).  When R is at most half a wave, the
// generated-loop kernel computes the first T − R raster ids (nblk) and smaller blocks the other R tiles — 6144^3: 2.25 waves -> 2 + a short one
// instead of 3 (profiles/r3e_hgemm_tail.log).  (knob 3 / 4: the remainder up to 0.75 / 1.0 of the CUs instead of 0.5 — A/B of the threshold,
// profiles/r6l_hgemm_tail_mid.log.)  Round 6 (knob 1, the default; 2 = round 5's 128-tile kernel + split-K, tmw = 0): where `mid_ok` the
// left-out tiles run on the mid-size kernel as 64 x 128 eighths while those fit ONE round of the CUs (R <= ncu / 8: twice the workgroups of the
// quadrants on CUs that would otherwise idle), else as 128 x 128 quadrants (lc_tune_set "hgemm_tail_tile" = `tile_knob`: 1 / 2 force
// either) — three ring slots when they fit one round of the CUs, two slots at two workgroups per CU beyond; no workspace, no reduce launch,
// legal under graph capture (+ 3 ... 7 % at 4352 ... 4864, 6144, 10240).
TailSplit tail_split(int knob, int tile_knob, bool mid_ok, int T, int ncu) {
  const int R = T % ncu;
  TailSplit t{-1, R, 0, 0};
  if (knob == 0 || T <= ncu || R == 0 || !(knob == 3 ? 4 * R <= 3 * ncu : knob == 4 || 2 * R <= ncu)) return t;
  t.nblk = T - R;
  if (mid_ok && knob != 2) {
    t.tmw = tile_knob == 1 ? 1 : tile_knob == 2 ? 2 : (8 * R <= ncu ? 1 : 2);
    t.ns = (t.tmw == 1 ? 8 : 4) * R <= ncu ? 3 : 2;
  }
  return t;
}

}  // namespace

// Shapes (the reference's kernels are legal on M, N multiples of 128 and K multiples of 32, hgemm_mma_stage.cu:650,675-676):
//   hgemm_w4y_kernel        M, N % 128 == 0 with a 256-tileable interior (the 128-wide border strips run on the 128-tile kernel),
//                           K % 32 == 0, K >= 64 (K % 64 == 32: a half K-step behind the generated loop)
//   hgemm_mfma128_kernel    M, N % 128 == 0, K % 32 == 0, K >= 64
//   the other 256-tile kernels (cross-checks): M, N % 256 == 0, K % 64 == 0
// Returns LC_OK or LC_ERR_SHAPE (an explicit family on a shape it does not take).
int plan_hgemm(const Knobs& k, int M, int N, int K, bool b_kn, int variant, bool al, HgemmPlan* out) {
  HgemmPlan p{};
  p.k = k;
  p.variant = variant;
  p.sched = b_kn ? 1 : k.w4y_sched;   // (the NN loop has one schedule)
  p.tail = TailSplit{-1, 0, 0, 0};
  const bool k64 = K % BK == 0, k32 = K % 32 == 0 && K >= BK;
  const bool tiles256 = (M % BM == 0) && (N % BN == 0) && k64 && al;
  const bool tiles128 = (M % BM1 == 0) && (N % BN1 == 0) && k32 && al;
  const bool edge_ok = al && K % 8 == 0 && (!b_kn || N % 8 == 0);   // hgemm_edge_kernel: whole 16-byte chunks
  // hgemm_w4y_kernel itself (not the 64-bit-address kernel w4_effective_variant substitutes for huge operands) on this shape
  const bool w4y_ok = tiles128 && M >= BM && N >= BN && w4_effective_variant(LC_HGEMM_MFMA256W4Y, b_kn, N, K) == LC_HGEMM_MFMA256W4Y;
  if (variant == LC_HGEMM_AUTO) {
    // measured crossover on MI355X (TN, square): the 256-tile kernel wins once its grid has more
    // than ~128 workgroups (n >= 3072); below that the 128-tile kernel fills the 256 CUs better
    // (n = 2048: 715 vs 436 TFLOP/s).
    const long wg256 = (long)(M / BM) * (N / BN), rcu = rule_cus(k);
    const bool tiles64 = (M % 64 == 0) && (N % 64 == 0) && k32 && al;
    p.mid = mid_tile_auto(k, M, N, K, b_kn, true);
    if (2 * wg256 > rcu && (tiles256 || (k.hgemm_auto == LC_HGEMM_MFMA256W4Y && w4y_ok))) {   // more than half a CU's worth of 256 x 256 tiles per CU (256 CUs: > 128)
      // ... unless those tiles leave CUs idle in their ONE round and a mid-size tile fills more of them in one round of its own
      // (3072^3 TN: 144 tiles of 256 x 256 against 256 of 192 x 192, 1050 -> 1110 TFLOP/s, profiles/r6p_hgemm_rect_splitk.log)
      p.fam = wg256 < rcu && p.mid.tmw > 0 && p.mid.wgs > wg256 ? HFam::MID : HFam::TILE256;
      p.variant = k.hgemm_auto;
    } else {
      // ragged M / N whose interior fills the flagship kernel: that kernel + a border launch, ahead of a 64-multiple tile of the mid-size kernel
      // (8192 x 8256 x 4096 TN: 1261 against 1096 TFLOP/s on 128 x 192 tiles, profiles/r6ab_hgemm_edge_ab.log)
      p.rag = tiles128 ? RaggedPlan{0, 0, 0, 0, 0, 0, 1} : ragged_plan(k, M, N, K, al, b_kn, true);
      if (p.rag.kind == 1) p.fam = HFam::RAGGED;
      else if (tiles64 && p.mid.tmw > 0) p.fam = HFam::MID;   // the tile with the least work on the busiest CU (n = 1280 .. 2816 square)
      else if (tiles128) p.fam = HFam::MFMA128;
      else if (p.rag.kind) p.fam = HFam::RAGGED;   // the whole problem on 128 x 128 tiles of the mid-size kernel that may reach beyond M / N
      else if ((p.Kp = kpad_plan(k, M, N, K, al, true))) p.fam = HFam::KPAD;   // K % 32 != 0 on a large problem: zero-padded operand copies + the tuned kernels
      else p.fam = edge_ok ? HFam::EDGE : HFam::GENERIC;
    }
  } else if (is_valu_variant(variant)) {   // a rung of the vector-ALU ladder (NN only): its own tile, else the generic kernel (never an error)
    int tm, tn, tk;
    valu_rung_tile(variant, &tm, &tn, &tk);
    const bool ok = (M % tm == 0) && (N % tn == 0) && (K % tk == 0) && (variant == LC_HGEMM_VALU_NAIVE || (al && K % 8 == 0));
    p.fam = ok && b_kn ? HFam::VALU : HFam::GENERIC;
  } else {   // an explicit family, on the shapes it takes
    bool ok = true;
    switch (variant) {
      case LC_HGEMM_GENERIC: p.fam = HFam::GENERIC; break;
      case LC_HGEMM_MFMA128: p.fam = HFam::MFMA128; ok = tiles128; break;
      case LC_HGEMM_EDGE: p.fam = HFam::EDGE; ok = edge_ok; break;
      case LC_HGEMM_MID: p.fam = HFam::MID; p.mid = mid_tile_auto(k, M, N, K, b_kn, false); ok = al && p.mid.tmw > 0; break;
      case LC_HGEMM_RAGGED: p.fam = HFam::RAGGED; p.rag = ragged_plan(k, M, N, K, al, b_kn, false); ok = p.rag.kind != 0; break;
      case LC_HGEMM_KPAD: p.fam = HFam::KPAD; p.Kp = kpad_plan(k, M, N, K, al, false); ok = p.Kp > 0; break;
      default: p.fam = HFam::TILE256; ok = tiles256 || (variant == LC_HGEMM_MFMA256W4Y && w4y_ok);   // (the 256-tile families)
    }
    if (!ok) return LC_ERR_SHAPE;
  }

  const int ncu = device_cu_count();   // (the tail rule sizes rounds with the device's own CU count)
  if (p.fam == HFam::TILE256) {
    p.tiles_m = M / BM;
    p.tiles_n = N / BN;
    if (is_w4_variant(p.variant)) {
      // M, N % 256 == 128 (hgemm_w4y_kernel only): the 128-wide right / bottom border strips go to the 128-tile kernel in the launch that
      // also takes the ragged last round unless the mid-size kernel does
      p.w4 = w4_effective_variant(p.variant, b_kn, N, K);
      p.nright = (N % BN) ? M / BM1 : 0;
      p.nbottom = (M % BM) ? 2 * p.tiles_n : 0;
      if (p.w4 == LC_HGEMM_MFMA256W4Y)
        p.tail = tail_split(k.hgemm_tail, k.hgemm_tail_tile, !p.nright && !p.nbottom && k.hgemm_mid != 1 && K < (1 << 22) && N < (1 << 22),
                            p.tiles_m * p.tiles_n, ncu);
      p.nb128 = p.tail.tmw ? 0 : (p.tail.nblk >= 0 ? 4 * p.tail.R : 0) + p.nright + p.nbottom;
      // Split-K of these blocks (lc_tune_set "hgemm_splitk"): a lone 128-tile block walks its K range at a quarter of a CU's MFMA rate
      // (one barrier per K tile, nothing to overlap with), and the launch holds few of them — 8192 x 8320 x 8192: 64 blocks, 107 us
      // for 1.5 % of the FLOPs (profiles/r5a_hgemm_shapes.log).  ks blocks per tile (about 1.5 per CU, each
      // range >= 8 K tiles) write fp32 partials into this stream's cached workspace, a second kernel adds them and stores C.
      if (p.nb128) {
        const int knob = k.hgemm_splitk, KT = K / BK;   // auto: ~1.5 blocks per CU (profiles/r5b_hgemm_splitk_sweep.log: 64 blocks: 4 best, 129 blocks: 3 best)
        p.ks = std::min(8, knob >= 2 ? knob : knob == 0 && p.nb128 < ncu ? (3 * ncu / 2 + p.nb128 / 2) / p.nb128 : 1);
        while (p.ks > 1 && KT / p.ks < 8) --p.ks;
        p.ksw = mfma128_ksw(k, p.nb128);   // (no workspace and few blocks: the eight-wave form of the kernel is the next best thing)
      }
    }
  } else if (p.fam == HFam::MFMA128) {
    p.ksw = mfma128_ksw(k, (long)(M / BM1) * (N / BN1));
  } else if (p.fam == HFam::RAGGED && p.rag.kind == 1) {
    p.w4 = LC_HGEMM_MFMA256W4Y;
    p.tiles_m = M / BM;
    p.tiles_n = N / BN;
    const int T = p.tiles_m * p.tiles_n, R = T % ncu;
    // the interior's last round: the default rule only (no 128-tile kernel here, no A/B thresholds or sub-tiles)
    p.tail = tail_split(k.hgemm_tail == 1 && k.hgemm_mid != 1, 0, true, T, ncu);
    // Fork rule (lc_tune_set "hgemm_ragged_fork"; profiles/r6ac … r6af_hgemm_edge_ab*.log; the hardware interleaves the two queues whatever their order or
    // priority): beside an interior of FULL rounds every CU a border block holds costs the interior a round of its own (4100 x 4104 x 4096, one round of
    // 256 tiles: 1122 -> 995 TFLOP/s; 12808^2 x 4096: − 5 %); beside an UNSPLIT last round that leaves at least 3 / 8 of the CUs idle the border fills them
    // (5200^2 x 4096, 400 tiles: 1182 -> 1234); beside a last round the mid-size kernel takes as quadrants it is a wash (5000^2 x 4096 − 4 %,
    // 777 x 50264 x 4096 + 3 %): not forked.
    const int fk = k.hgemm_ragged_fork;
    p.fork = fk == 2 || (fk == 0 && p.tail.nblk < 0 && R > 0 && 8 * (ncu - R) >= 3 * ncu);
  }
  *out = p;
  return LC_OK;
}

// The variant a reference entry name runs (lc_hgemm_call): the cross-check kernels need 256-multiples and K % 64 == 0; every reference entry must still accept the
// reference's own legal shapes (multiples of 128 / K of 32, hgemm_mma_stage.cu:650,675), so fall back per shape: AUTO serves those with the flagship kernel + border
// strips, the 128-tile kernel or the edge kernel (plan_hgemm).
// Round 6: the entry names that map to the cross-check kernels keep them where those kernels are within a few per cent of the flagship
// (large grids: the reference bench's rows stay distinct there), but a 256 x 256 tile on a grid of at most half a CU's worth of tiles
// per CU — 2048^3: 64 workgroups, 330 TFLOP/s where LC_HGEMM_AUTO reaches 818 in the reference's own unmodified sweep
// (profiles/r6Z_f1_hgemm_default_sweep.log) — serves nobody: such calls, and 128-tile names on shapes the mid-size kernel serves, run
// what LC_HGEMM_AUTO runs.  (LC_HGEMM_AUTO, LC_HGEMM_GENERIC and the vector-ALU rungs run as the table says on every shape.)
int hgemm_entry_variant(const Knobs& k, const HgemmEntry& e, int M, int N, int K, bool al) {
  int variant = e.variant;
  const bool tiles256 = (M % BM == 0) && (N % BN == 0) && (K % BK == 0) && al;
  const bool tiles128 = (M % BM1 == 0) && (N % BN1 == 0) && (K % 32 == 0) && K >= BK && al;
  if (is_tile256_variant(variant) && !tiles256) variant = LC_HGEMM_AUTO;
  if (variant == LC_HGEMM_MFMA128 && !tiles128) variant = LC_HGEMM_GENERIC;
  if (is_tile256_variant(variant) && variant != LC_HGEMM_MFMA256W4Y && 2L * (M / BM) * (N / BN) <= rule_cus(k)) variant = LC_HGEMM_AUTO;
  HgemmPlan p;
  const bool plans = variant == LC_HGEMM_MFMA128 && M > 0 && N > 0 && K > 0 && plan_hgemm(k, M, N, K, e.layout == LC_LAYOUT_NN, LC_HGEMM_AUTO, al, &p) == LC_OK;
  return plans && p.fam == HFam::MID ? LC_HGEMM_AUTO : variant;
}

int plan_gemm_fp8(const Knobs& k, const GemmFp8Call& c, GemmFp8Plan* p) {   // the fp8 / MX GEMM entries (lc_plan.h GemmFp8Call / GemmFp8Plan)
  const bool fits = w4_rows_fit(c.K, 1);
  if (c.mx && !fits) return LC_ERR_SHAPE;   // 32-bit DMA offsets (K < 8 Mi) of the one kernel that takes block scales
  const Fp8Kern kern = c.mx ? Fp8Kern::W4K_MX : k.fp8_mx == 0 ? Fp8Kern::PINGPONG2 : k.fp8_mx == 2 || !fits ? Fp8Kern::PINGPONG2_MX : k.fp8_mx == 3 ? Fp8Kern::W4K : Fp8Kern::W4;
  *p = GemmFp8Plan{kern, c.M / BM, c.N / BN, panel_tiles(k.hgemm_raster, c.swizzle_stride, c.N / BN, BN, ((size_t)c.M + c.N) * c.K), c};   // (fp8: one byte per element)
  return LC_OK;
}
int check_gemm_fp8(const GemmFp8Call& c, const GemmFp8Ptrs* a, GemmFp8Plan* p) {
  if (a && (!a->A || !a->B || !a->C || (c.mx && (!a->PA || !a->PB)))) return LC_ERR_ARG;
  if (c.M <= 0 || c.N <= 0 || c.K <= 0 || c.M % BM || c.N % BN || c.K % 128) return LC_ERR_SHAPE;
  if (a && (!aligned16(a->A) || !aligned16(a->B) || !aligned16(a->C) || (c.mx && (!aligned8(a->PA) || !aligned8(a->PB))))) return LC_ERR_SHAPE;
  return plan_gemm_fp8(read_knobs(), c, p);
}

// The name of what a plan launches (lc_hgemm_kernel_name; bench.py, tools/ and the tests parse these strings).
void format_hgemm(const HgemmPlan& p, int M, int N, bool b_kn, char* buf, int buflen) {
  const char* nn = b_kn ? "true" : "false";
  switch (p.fam) {
    case HFam::VALU: snprintf(buf, buflen, "%s", valu_rung_kernel_name(p.variant)); return;
    case HFam::TILE256:
      if (p.w4 == LC_HGEMM_MFMA256W4X) snprintf(buf, buflen, "hgemm_w4x_kernel<%s>", nn);
      else if (p.w4 == LC_HGEMM_MFMA256W4Y) snprintf(buf, buflen, "hgemm_w4y_kernel<%s,%d>", nn, p.sched);
      else if (p.w4) snprintf(buf, buflen, "hgemm_w4b_kernel<%s,%s,0>", nn, p.w4 == LC_HGEMM_MFMA256W4B ? "false" : "true");
      else if (p.variant == LC_HGEMM_MFMA256P2) snprintf(buf, buflen, "hgemm_pingpong2_kernel<%s,false>", nn);
      else snprintf(buf, buflen, "hgemm_mfma256_kernel<%s>", nn);
      return;
    case HFam::MID:
      if (p.mid.ks > 1) snprintf(buf, buflen, "hgemm_mid_sk_kernel<%s,%d,%d> x%d", nn, p.mid.tmw, p.mid.ns, p.mid.ks);   // (x K ranges, + hgemm_mid_reduce_kernel; hgemm_mid_kernel under graph capture)
      else snprintf(buf, buflen, "hgemm_mid_kernel<%s,%d,%d,%d>", nn, p.mid.tmw, p.mid.tnw, p.mid.ns);
      return;
    case HFam::MFMA128: snprintf(buf, buflen, "hgemm_mfma128_kernel<%s,%d>", nn, p.ksw); return;
    case HFam::KPAD: {   // the copies + whatever the padded problem runs
      HgemmPlan inner;
      char name[160];
      plan_hgemm(p.k, M, N, p.Kp, b_kn, LC_HGEMM_AUTO, true, &inner);   // (LC_HGEMM_AUTO always has a plan)
      format_hgemm(inner, M, N, b_kn, name, (int)sizeof(name));
      snprintf(buf, buflen, "hgemm_pad_copy_kernel + %s", name);
      return;
    }
    case HFam::RAGGED:   // interior kernel + the border launch
      if (p.rag.kind == 1) snprintf(buf, buflen, "hgemm_w4y_kernel<%s,%d> + hgemm_mid_edge_kernel<%s,2,2,%d>", nn, p.sched, nn, p.rag.ns);
      else if (p.rag.ks > 1) snprintf(buf, buflen, "hgemm_mid_edge_sk_kernel<%s,%d,3> x%d", nn, p.rag.tmw, p.rag.ks);   // (x K ranges, + hgemm_mid_reduce_edge_kernel; hgemm_mid_edge_kernel under graph capture)
      else snprintf(buf, buflen, "hgemm_mid_edge_kernel<%s,%d,%d,%d>", nn, p.rag.tmw, p.rag.tnw, p.rag.ns);
      return;
    case HFam::EDGE: snprintf(buf, buflen, "hgemm_edge_kernel<%s>", nn); return;
    case HFam::GENERIC: snprintf(buf, buflen, "hgemm_generic_kernel<%s>", nn); return;
  }
}

namespace {
int attn_walk_auto(const Knobs& k, int N, int D) {
  // auto (lc_tune_set "attn_walk": 0 = this rule; measured, profiles/r3k, profiles/r4c_attn_walks.log, r5p_attn_walks.log): up to N = 4096 the
  // persistent static walk (round 3: config 3 + 1.7 %, N = 2048 + 1.0 %; later boxes: + 0.5 % / level), beyond it one block per workgroup —
  // with 16+ blocks per CU the hardware dispatcher balances better than either walk (D = 128, N = 8192: static - 1.0 %, dynamic queue - 1.1 %;
  // the queue is a validated alternative, never the default) — except D = 64, whose blocks are half as long: (1,48,8192,64) static + 1.4 %
  if (k.attn_walk >= 1 && k.attn_walk <= 3) return k.attn_walk - 1;
  return (N <= 4096 || (D == 64 && N <= 8192)) ? 1 : 0;
}
// Split-KV factor of the merged-phase kernel for a launch of `bh` (batch, head) problems (lc_tune_set "attn_split"; 1 = no split).
// The kernel owns 256 query rows per workgroup and one workgroup per CU, so g = bh N / 256 workgroups on ncu CUs run ceil(g / ncu)
// rounds of T = N / 64 KV tiles: a grid that does not fill the GPU (the reference author's own regime, README.md:120 "B <= 4, H <= 48,
// SeqLen <= 8192") leaves CUs idle for the whole launch, and a grid of 1.25 rounds pays for 2.  With S KV ranges per query block the
// launch runs ceil(g S / ncu) rounds of T / S tiles + the combine.  Auto picks, among S = 2, 4, 8, 16 (T divisible, >= kMinSplitTiles
// tiles per range, partials <= 256 MiB), the S that minimises the cost model
//     t(S) = ceil(g S / ncu) (T / S) tau_D + [S > 1] (x0 + S * 4 bh N D bytes / bw)          (microseconds)
// and splits when that is 5 % below t(1).  Fitted to profiles/r5b_attn_split.log, r5f_attn_split_quant.log, r5f_small_split_kernel_
// durations.log: tau_128 = 1.35, tau_64 = 0.85 us per 64-key tile of a 256-row block, x0 = 5 us (the combine kernel: 4.9 us), bw = the rate
// at which a range's fp16 partial is written and read back (2.6 TB/s: small transfers).  Examples (256 CUs): (1,8,1024,128) -> 4 (+ 34 %),
// (1,8,2048,64) -> 4 (+ 61 %), (1,4,4096,128) -> 4 (2.1 x), (1,2,8192,128) -> 8 (2.6 x), (1,16,2048,128) -> 2 (+ 20 %), (1,10,8192,128) -> 4
// (1.25 rounds: + 22 %), (1,12,8192,64) -> 2 (+ 18 %), (1,32,1024,128) -> 1 (a half-full GPU and 16 tiles: the combine costs more than
// half the walk saves), (1,6,8192,128) -> 1, config 3 / 4 -> 1.  bh < 0 (lc_attn_kernel_name has no batch / head count): no split.
constexpr int kMinSplitTiles = 4;
int attn_split_auto(const Knobs& kn, int D, int N, long bh) {
  const int k = kn.attn_split;
  if ((D != 128 && D != 64) || N % 256 != 0 || bh <= 0 || k == 1) return 1;
  const int T = N / 64;
  const double part = 4.0 * (double)bh * N * D;   // bytes of one range's partial O, written + read
  const double part_cap = 2.0 * ((size_t)256 << 20);   // partials <= 256 MiB, forced factor or auto (round-5 advisor: a forced 16 on config 4 asked for 34 GiB)
  if (k >= 2) return (T % k == 0 && T / k >= 2 && k * part <= part_cap) ? k : 1;
  const long ncu = rule_cus(kn), g = bh * (N / 256);
  // the model's constants: measured on this device (lc_tune_calibrate) or the values fitted on the round-5 boxes
  double tau = D == 128 ? 1.35 : 0.85, fixed_us = kSplitFixedUs, bytes_per_us = kSplitBytesPerUs;
  {
    int dev = 0;
    if (kn.attn_calib == 0 && kn.rule_cus == 0 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && g_attn_calib[dev].valid.load(std::memory_order_acquire)) {
      tau = D == 128 ? g_attn_calib[dev].tau128 : g_attn_calib[dev].tau64;
      fixed_us = g_attn_calib[dev].x0;
      bytes_per_us = g_attn_calib[dev].bytes_per_us;
    } else {
      (void)hipGetLastError();
    }
  }
  int best = 1;
  const double t1 = (double)((g + ncu - 1) / ncu) * T * tau;
  double tbest = 0.95 * t1;
  for (int S = 2; S <= 16 && T % S == 0 && T / S >= kMinSplitTiles && S * part <= part_cap; S *= 2) {
    const double t = (double)((g * S + ncu - 1) / ncu) * (T / S) * tau + fixed_us + S * part / bytes_per_us;
    if (t < tbest) {
      tbest = t;
      best = S;
    }
  }
  return best;
}
// D <= 128
AttnPlan choose_attn_nw(const Knobs& k, int D, bool vt, int N, long bh) {
  auto w4u = [](int walk, int ns) { AttnPlan p{}; p.kern = AKern::W4U; p.walk = walk; p.nsplit = ns; return p; };
  auto w4i = [&] { AttnPlan p{}; p.kern = AKern::W4I; p.sched = k.attn_w4i_sched; return p; };
  auto lockstep = [&](int nw) { AttnPlan p{}; p.kern = AKern::LOCKSTEP; p.nw = nw; p.abl = k.attn_ablate; return p; };
  const int want = k.attn_nw == 512 ? 513 : k.attn_nw;   // 0 = auto
  const bool merged = (D == 128 || D == 64) && N % 256 == 0;
  if (merged && k.attn_ablate == 0) {
    if (want == 0) {
      const int ns = attn_split_auto(k, D, N, bh);
      if (ns > 1) return w4u(3, ns);
      // Small grids the split rule leaves alone (too few KV tiles for the combine to pay): up to half a GPU of 256-row blocks and N <= 2048
      // the 4-wave lock-step kernel's 128-row workgroups fill twice the CUs — (1,32,1024,128) 655 vs 601 TFLOP/s, (1,32,1024,64) 498 vs 444
      // (profiles/r4q_small_grids_d128.log, r5i_small_grids.log); from one full round of blocks on the merged-phase kernel is far ahead (992 vs 760)
      if (bh > 0 && 2 * bh * (N / 256) <= rule_cus(k) && N <= 2048 && k.attn_split != 1) return lockstep(4);
      return w4u(attn_walk_auto(k, N, D), 1);
    }
    if (want == 513 || want == 515 || want == 517) return w4u(want == 513 ? 0 : want == 515 ? 1 : 2, 1);
    if (want == 514 && !vt) return w4i();
  }
  // N % 256 != 0 (N % 64 == 0; N % 128 == 0 is what the reference's own kernels need: flash_attn_mma_share_qkv.cu:839 asserts
  // N % max(Br, Bc) == 0): the merged-phase kernel with one block per workgroup, the head's last 256-row block partly real — the waves whose 64
  // rows lie behind N compute on a clamped copy of the last row and store nothing ((256 - N % 256) / (N + 256 - N % 256) of the work wasted).
  // From N = 1152 on that beats the lock-step kernel's MFMA-busy 0.46 vs 0.58 (profiles/r5d_attn_n128.log: (4,32,4224,128) 1210 vs 901 TFLOP/s,
  // (4,32,1152,128) 886 vs 771, (1,48,8320,64) 961 vs 799; (2,16,896,64) 372 vs 427: the lock-step kernel keeps N < 1152)
  if ((D == 128 || D == 64) && N % 256 != 0 && N % 64 == 0 && N >= 1152 && k.attn_ablate == 0 && (want == 0 || want == 513)) return w4u(0, 1);
  // D = 96 / 32: only the generated kernel (attn_w4i.hip) has a merged-phase instantiation (256-B / 128-B padded LDS rows)
  if ((D == 96 || D == 32) && !vt && N % 256 == 0 && (want == 0 || want >= 256)) return w4i();
  if (N % 256 == 0 && (want == 0 || want >= 8)) return lockstep(8);
  if (N % 128 == 0 && (want == 0 || want >= 4)) return lockstep(4);
  return lockstep(2);
}

// causal, D <= 128: the causal merged-phase kernel for D = 64 / 128, N % 256 == 0 unless "attn_nw" = 8 / 4 / 2 forces the lock-step kernel
// (the independent cross-check); everything else: the causal lock-step kernel with the waves the non-causal rule gives.  Neither splits KV
// or switches kernels by grid size, so a causal result does not depend on B x H or the CU count.  Grid order of the merged-phase kernel
// (p.order: 0 = longest block first, 1 = head-major; same bits): longest first up to 8 rounds of blocks per CU — the dispatcher then
// fills the tail with short blocks: (4,32,4096,128) 1042 vs 977 TFLOP/s, (1,48,8192,64) 983 vs 851 —, head-major beyond, where the K / V
// of the heads in flight no longer fit L2: (8,32,8192,128), 32 rounds, 1143 vs 954; config 4 1140 vs 926.  bh < 0: no
// launch, no order.
AttnPlan choose_attn_causal(const Knobs& k, int D, int N, long bh) {
  AttnPlan p{};
  const int want = k.attn_nw;
  if ((D == 128 || D == 64) && N % 256 == 0 && want != 8 && want != 4 && want != 2) {
    p.kern = AKern::W4U_CAUSAL;
    const int o = k.attn_causal_order;
    p.order = o == 1 ? 0 : o == 2 ? 1 : (bh > 0 && bh * (N / 256) > 8L * rule_cus(k)) ? 1 : 0;
    return p;
  }
  p.kern = AKern::LOCKSTEP_CAUSAL;
  p.nw = N % 256 == 0 && (want == 0 || want >= 8) ? 8 : N % 128 == 0 && (want == 0 || want >= 4) ? 4 : 2;
  return p;
}

// D = 256 / 512 with N % 128 == 0: the full-width kernel (attn_bigd2.hip; V as [B,H,N,D], or — D = 256, the reach of the reference's
// *_swizzle_qkv entries — as [B,H,D,N]) unless lc_tune_set "attn_d512" = 1 asks for round 1's column-split kernel (kept as the
// independently written cross-check; it also serves N % 128 != 0 and D = 512 with V transposed).  D = 1024 with N % 64 == 0: the pair
// kernel (attn_bigd4.hip); the column-split kernel under knob 1 and for ragged N.
bool use_bigd2(const Knobs& k, int D, bool vt, int N) {
  return (D == 256 || (D == 512 && !vt)) && N % 128 == 0 && k.attn_d512 != 1;   // (2: attn_bigd3, same launcher; not for vt)
}
bool use_bigd4(const Knobs& k, int D, bool vt, int N) { return D == 1024 && !vt && N % 64 == 0 && k.attn_d512 != 1; }
// D = 512: attn_bigd6 (16x16x32 MFMAs) or attn_bigd2 (32x32x16): kBigd6Auto says which one auto means, knob 3 selects the other
constexpr bool kBigd6Auto = true;    // profiles/r4k_bigd6.log: fp16 + 3.4 ... 4.7 %, bf16 + 1.8 ... 2.8 % at the cap (zero-filled: - 8 %, the 16-wide stream is more issue-bound)
bool use_bigd6(const Knobs& kn, int D, bool vt, int N) {
  const int k = kn.attn_d512;
  return D == 512 && !vt && N % 128 == 0 && (((k == 0 || k == 4) && kBigd6Auto) || (k == 3 && !kBigd6Auto));
}
// D = 256 with N % 256 == 0, either V layout: attn_bigd7 (64 query rows per wave, 16x16x32 MFMAs, KV rings) is auto; knob 3 selects
// attn_bigd2 (32 rows per wave, 32x32x16: the cross-check on the other MFMA shape, and the kernel for N % 256 == 128)
// attn_bigd7's workgroup owns 256 query rows, attn_bigd2's 128: on a grid that does not fill the GPU the smaller blocks win (measured,
// profiles/r4p_bigd7_small_grids.log: (1,8,1024,256) 156 vs 272 TFLOP/s, (1,16,2048,256) 693 vs 978; from 192 workgroups up attn_bigd7 is
// ahead).  With g7 = B H N / 256 workgroups of attn_bigd7 (1.6 time units each: twice the rows at 0.8 of the time per FLOP) against 2 g7 of
// attn_bigd2 (1 unit each), rounds of one workgroup per CU: attn_bigd7 iff 1.6 ceil(g7 / CUs) <= ceil(2 g7 / CUs), and always from 4 rounds up.
// bh < 0: "a grid that fills the GPU" (lc_attn_kernel_name has no batch / head count; lc_attn_kernel_name_bh has).  Knob 4 forces attn_bigd7 (tests of small shapes).
bool use_bigd7(const Knobs& kn, int D, bool vt, int N, long bh) {
  const int k = kn.attn_d512;
  // N % 256 == 128 (round 5): the 256-row kernel with its last block half real, from N = 1152 (below, attn_bigd2's 128-row workgroups waste nothing)
  if (D != 256 || (N % 256 != 0 && (N % 256 != 128 || N < 1152)) || (k != 0 && k != 4)) return false;
  if (k == 4 || bh < 0) return true;
  const long ncu = rule_cus(kn), g7 = bh * ((N + 255) / 256);
  if (g7 >= 4 * ncu) return true;
  const long c7 = (g7 + ncu - 1) / ncu, c2 = (2 * g7 + ncu - 1) / ncu;
  return 16 * c7 <= 10 * c2;
}

}  // namespace

// ONE decision per attention call (lc_attn_fwd_f16 / _bf16 / _f16_ex / _f16_gqa launch it, lc_attn_kernel_name_bh / _ex / _gqa report it; bf16
// launches have V as [B,H,N,D]; causal: fp16, D <= 128), kept in the plan with the call it was made for (c.gqa decides nothing here).  Returns
// LC_OK or LC_ERR_HEADDIM.
int plan_attn(const Knobs& k, const AttnCall& c, AttnPlan* p) {
  const long bh = c.bh;
  const int N = c.N, D = c.D;
  const bool vt = c.vt, bf16 = c.bf16;
  if (is_small_headdim(D)) {
    if (bf16) return LC_ERR_HEADDIM;
    *p = c.causal ? choose_attn_causal(k, D, N, bh) : choose_attn_nw(k, D, vt, N, bh);
    p->call = c;
    return LC_OK;
  }
  if (c.causal) return LC_ERR_HEADDIM;
  *p = AttnPlan{};
  p->call = c;
  p->span8 = k.attn_d1024;
  p->nw = N % 128 == 0 ? 4 : 2;
  if (use_bigd4(k, D, vt, N) && !bf16) p->kern = AKern::BIGD4;
  else if (use_bigd6(k, D, vt, N)) p->kern = AKern::BIGD6;
  else if (use_bigd7(k, D, vt, N, bh) && !(bf16 && vt)) p->kern = AKern::BIGD7;
  else if (use_bigd2(k, D, vt, N) && !(bf16 && vt)) p->kern = !vt && k.attn_d512 == 2 ? AKern::BIGD3 : AKern::BIGD2;   // (bigd3: experimental 32-row double-buffered tiles)
  else if (D == 256 || D == 512 || (D == 1024 && !bf16)) p->kern = AKern::COLSPLIT;
  else return LC_ERR_HEADDIM;
  return LC_OK;
}

// Decode attention (lc_plan.h DecodeCall / DecodePlan).  The auto rule: a workgroup streams its range at a rate that does not depend on the grid, so the call is as
// fast as its longest range once every CU has a workgroup — the smallest S with B Hkv S >= CUs — and a range shorter than 4 tiles (one per wave) leaves
// waves without work while the combine still reads S partials.
int plan_attn_decode(const Knobs& k, const DecodeCall& c, DecodePlan* p) {
  const long R = (long)(c.H / c.Hkv) * c.Nq;   // (> 64: a chunk call)
  p->call = c;
  p->cache = !c.paged ? DecodeCache::FLAT : c.kv_bytes == 1 ? DecodeCache::PAGED_KV8 : DecodeCache::PAGED;
  p->Ncap = c.paged ? c.max_pages * c.page_size : c.Ncap;
  p->RT = R <= 16 ? 1 : R <= 32 ? 2 : 4;
  p->RB = (int)((R + 63) / 64);   // row blocks: each is a workgroup per KV range, and counts as a group of the rule
  p->local = c.window > 0 || c.sinks;
  p->S = k.attn_decode_split;
  if (p->S > 0) return LC_OK;
  // (a window: a workgroup walks at most window + Nq - 1 keys and the rest of the tile its lowest one lies in — not kv_len's business either)
  const long walked = c.window > 0 ? std::min((long)p->Ncap, (long)c.window + c.Nq - 1 + 63) : (long)p->Ncap;
  long groups = (long)c.B * c.Hkv * p->RB;
  // (varlen: no more row blocks hold work than the T tokens can fill — ceil(G T / 64) full ones and a partial one per sequence — whatever cu_q says)
  if (c.varlen) groups = c.Hkv * std::min((long)c.B * p->RB, ((long)(c.H / c.Hkv) * c.T + 63) / 64 + c.B);
  const long tiles = (walked + 63) / 64;
  long S = (rule_cus(k) + groups - 1) / groups;
  S = std::min(S, tiles / 4);
  p->S = (int)std::max(1L, std::min(S, 64L));
  return LC_OK;
}
int check_attn_decode(const DecodeCall& c, const DecodePtrs* a, DecodePlan* p) {
  if (c.flags & ~LC_ATTN_CAUSAL) return LC_ERR_ARG;   // (LC_ATTN_V_TRANSPOSED: a cache grows along N, there is no [D,N] cache)
  if (c.window < 0 || ((c.window > 0 || c.tree) && !(c.flags & LC_ATTN_CAUSAL))) return LC_ERR_ARG;   // a window is a lower edge of the causal mask, a tree mask (§4.3o) a set of holes in it
  if (a && (!a->Q || !a->K || !a->V || !a->O || (c.paged && (!a->block_table || !a->kv_len)) || (c.varlen && !a->cu_q) || (c.lse && !a->lse) || (c.tree && !a->tree_mask))) return LC_ERR_ARG;   // (k_scale / v_scale: NULL = 1.0)
  if (c.H <= 0 || c.Hkv < 1 || c.Hkv > c.H || c.H % c.Hkv != 0) return LC_ERR_SHAPE;
  if (c.B <= 0 || c.Nq <= 0 || c.D <= 0) return LC_ERR_SHAPE;
  if (c.varlen && (c.T < 1 || c.max_nq > c.T)) return LC_ERR_SHAPE;   // (Nq IS max_nq: < 1 is refused above)
  long ncap = c.Ncap;
  if (c.paged) {
    if (c.num_pages <= 0 || c.max_pages <= 0) return LC_ERR_SHAPE;
    if (c.page_size < 16 || (c.page_size & (c.page_size - 1)) != 0) return LC_ERR_SHAPE;   // a power of two >= 16: a 16-key load group never straddles a page
    ncap = (long)c.max_pages * c.page_size;
    if (ncap > 0x7fffffffL) return LC_ERR_SHAPE;
  } else if (ncap <= 0) return LC_ERR_SHAPE;
  // R = G x Nq query rows per K / V head: four row tiles of 16 — a chunk entry has ceil(R / 64) row blocks of them instead
  const long R = (long)(c.H / c.Hkv) * c.Nq;
  if (!c.chunk && R > 64) return LC_ERR_SHAPE;
  // one head's Ncap rows (an upper bound of one page run) stay below 2 GiB: the kernel's 32-bit offsets (attn_span_fits at kv_bytes an element)
  if ((size_t)ncap * (size_t)c.D * (size_t)c.kv_bytes >= 0x80000000ull) return LC_ERR_SHAPE;
  if ((size_t)c.B * c.Hkv * (size_t)((R + 63) / 64) * 64 > 0x7fffffffull) return LC_ERR_SHAPE;   // 1-D grid of B x Hkv x RB x S workgroups, S <= 64
  if (a && (!aligned16(a->Q) || !aligned16(a->K) || !aligned16(a->V) || !aligned16(a->O) || (c.tree && !aligned8(a->tree_mask)))) return LC_ERR_SHAPE;
  if (c.D != 64 && c.D != 128) return LC_ERR_HEADDIM;
  return plan_attn_decode(read_knobs(), c, p);
}
void format_attn_decode(const DecodePlan& p, char* buf, int buflen) {
  static const char* const kKernels[] = {"attn_decode_kernel", "attn_decode_paged_kernel", "attn_decode_paged_kv8_kernel"};   // by DecodeCache
  static const char* const kLocal[] = {"attn_local_kernel", "attn_local_paged_kernel", "attn_local_paged_kv8_kernel"};
  const char* kern = (p.local ? kLocal : kKernels)[(int)p.cache];
  char ragged[64];
  if (p.call.varlen) {   // attn_varlen_ [chunk_] paged_ [kv8_] [lse_ | tree_] [bf16_] kernel, from the fields the launch is reached by (bf16, lse, tree: varlen only)
    snprintf(ragged, sizeof ragged, "attn_varlen_%spaged_%s%s%skernel", p.RB > 1 ? "chunk_" : "", p.cache == DecodeCache::PAGED_KV8 ? "kv8_" : "",
             p.call.tree ? "tree_" : p.call.lse ? "lse_" : "", p.call.bf16 ? "bf16_" : "");
    kern = ragged;
  }
  if (p.RB > 1) {   // (the chunk kernels have four row tiles and say so nowhere)
    static const char* const kChunk[] = {"attn_chunk_kernel", "attn_chunk_paged_kernel", "attn_chunk_paged_kv8_kernel"};
    static const char* const kLocalChunk[] = {"attn_local_chunk_kernel", "attn_local_chunk_paged_kernel", "attn_local_chunk_paged_kv8_kernel"};
    const char* chunk = p.call.varlen ? kern : (p.local ? kLocalChunk : kChunk)[(int)p.cache];
    if (p.S > 1) snprintf(buf, buflen, "%s<%d> x%d", chunk, p.call.D, p.S);
    else snprintf(buf, buflen, "%s<%d>", chunk, p.call.D);
    return;
  }
  if (p.S > 1) snprintf(buf, buflen, "%s<%d,%d> x%d", kern, p.call.D, p.RT, p.S);   // (x KV ranges, + attn_decode_combine_kernel<D>)
  else snprintf(buf, buflen, "%s<%d,%d>", kern, p.call.D, p.RT);
}

// The merge of two attention states (lc_plan.h MergeCall): the statuses of the decode entries, in their order — a NULL pointer (cu_q may be one),
// the shape, the alignment of the 16-byte lanes, the head dim.
int check_attn_merge(const MergeCall& c, const MergePtrs& p) {
  if (!p.Oa || !p.lse_a || !p.Ob || !p.lse_b || !p.Oout || !p.lse_out) return LC_ERR_ARG;
  if (c.B < 1 || c.T < 1 || c.H < 1 || c.D <= 0) return LC_ERR_SHAPE;
  if ((long)c.T * c.H > 0x7fffffffL) return LC_ERR_SHAPE;   // rows are counted in 32 bits by the grid
  if (!aligned16(p.Oa) || !aligned16(p.Ob) || !aligned16(p.Oout)) return LC_ERR_SHAPE;
  if (c.D != 64 && c.D != 128) return LC_ERR_HEADDIM;
  return LC_OK;
}

// Append to the paged cache (lc_plan.h AppendCall).  The page geometry and the span bound are check_attn_decode's, so that every pool an append
// accepts is one the decode call of the same step accepts; Nq is not bounded by the decode kernel's row tiles: a prefill writes whole prompts.
int check_kv_append(const AppendCall& c, const AppendPtrs* a) {
  if (c.flags != 0) return LC_ERR_ARG;   // no flag is defined
  if (a && (!a->Knew || !a->Vnew || !a->Kpool || !a->Vpool || !a->block_table || !a->kv_len)) return LC_ERR_ARG;   // (k_scale / v_scale: NULL = 1.0)
  if (c.B <= 0 || c.Hkv <= 0 || c.Nq <= 0 || c.num_pages <= 0 || c.max_pages <= 0 || c.D <= 0) return LC_ERR_SHAPE;
  if (c.page_size < 16 || (c.page_size & (c.page_size - 1)) != 0) return LC_ERR_SHAPE;
  const long ncap = (long)c.max_pages * c.page_size;
  if (ncap > 0x7fffffffL) return LC_ERR_SHAPE;
  // one (page, head) run stays below 2 GiB — the kernel's 32-bit offsets inside a run — by the decode calls' bound on Ncap rows
  if ((size_t)ncap * (size_t)c.D * (size_t)c.kv_bytes >= 0x80000000ull) return LC_ERR_SHAPE;
  // 1-D grid of B x Hkv x ceil(Nq / tokens per workgroup) workgroups (each factor < 2^31: no product here overflows 64 bits)
  const size_t bh = (size_t)c.B * c.Hkv;
  if (bh > 0x7fffffffull || bh * (((size_t)c.Nq - 1) / kv_append_tokens_per_block(c.D) + 1) > 0x7fffffffull) return LC_ERR_SHAPE;
  if (a && (!aligned16(a->Knew) || !aligned16(a->Vnew) || !aligned16(a->Kpool) || !aligned16(a->Vpool))) return LC_ERR_SHAPE;
  if (c.D != 64 && c.D != 128) return LC_ERR_HEADDIM;
  return LC_OK;
}
void format_kv_append(const AppendCall& c, char* buf, int buflen) {
  snprintf(buf, buflen, c.kv_bytes == 1 ? "kv_append_paged_kv8_kernel<%d>" : "kv_append_paged_kernel<%d>", c.D);
}

// Rotary embedding + append (lc_plan.h RopeAppendCall).  Its own ARG checks first, then check_kv_append for everything the two calls share; a
// head dim append refuses is reported only after every SHAPE check of this call has passed (ARG, SHAPE, HEADDIM: the order of every entry).
// A varlen call (c.varlen): LC_ROPE_PACKED_SRC is an unknown flag (the two strides say it all), cu_q joins the NULL check, T and max_nq the
// shape check; the strides are those of token-major rows; the grid is ceil(T / tokens per workgroup) x (Hkv + H).  (check_kv_append sees
// Nq = max_nq: its grid bound is that of the rectangular call the ragged one replaces.)
int check_rope_append(const RopeAppendCall& c, const RopeAppendPtrs* p) {
  if (c.flags & ~(c.varlen ? LC_ROPE_INTERLEAVED : LC_ROPE_INTERLEAVED | LC_ROPE_PACKED_SRC)) return LC_ERR_ARG;
  if (p && (!p->Q || !p->Qout || !p->cos_sin || (c.varlen && !p->cu_q) || (c.pos && !p->pos_ids))) return LC_ERR_ARG;
  const int rc = check_kv_append(c.a, p ? &p->a : nullptr);
  if (rc != LC_OK && rc != LC_ERR_HEADDIM) return rc;
  const int D = c.a.D;
  if (c.H <= 0 || c.max_pos <= 0 || c.H % c.a.Hkv != 0) return LC_ERR_SHAPE;
  if (c.rot_dim < 16 || c.rot_dim > D || c.rot_dim % 16 != 0) return LC_ERR_SHAPE;   // a NeoX partner is a whole 16-byte chunk away
  if (c.varlen) {
    if (c.T < 1 || c.max_nq > c.T) return LC_ERR_SHAPE;
    if (c.src_row_stride % 8 != 0 || c.src_row_stride < (long long)c.H * D) return LC_ERR_SHAPE;
    if (c.kv_row_stride % 8 != 0 || c.kv_row_stride < (long long)c.a.Hkv * D) return LC_ERR_SHAPE;
    if (((size_t)c.T - 1) / kv_append_tokens_per_block(D) + 1 > 0x7fffffffull / ((size_t)c.a.Hkv + (size_t)c.H)) return LC_ERR_SHAPE;
    if (p && (!aligned16(p->Q) || !aligned16(p->Qout))) return LC_ERR_SHAPE;
    if (p && p->Q == p->Qout && c.src_row_stride != (long long)c.H * D) return LC_ERR_SHAPE;   // in place: the dense layout only
    return rc;
  }
  if (c.flags & LC_ROPE_PACKED_SRC) {
    if (c.src_row_stride % 8 != 0 || c.src_row_stride < ((long long)c.H + 2LL * c.a.Hkv) * D) return LC_ERR_SHAPE;
  } else if (c.src_row_stride != 0) return LC_ERR_SHAPE;
  // 1-D grid of (B x Hkv + B x H) x ceil(Nq / tokens per workgroup) workgroups
  const size_t bh = (size_t)c.a.B * ((size_t)c.a.Hkv + (size_t)c.H);
  if (bh > 0x7fffffffull || bh * (((size_t)c.a.Nq - 1) / kv_append_tokens_per_block(D) + 1) > 0x7fffffffull) return LC_ERR_SHAPE;
  if (p && (!aligned16(p->Q) || !aligned16(p->Qout))) return LC_ERR_SHAPE;
  return rc;
}
void format_rope_append(const RopeAppendCall& c, char* buf, int buflen) {
  // rope_append_paged_ [kv8_] kernel; a varlen call: rope_append_varlen_ [pos_] [kv8_] [bf16_] kernel (bf16: §4.3m, pos: §4.3o — varlen only)
  snprintf(buf, buflen, "rope_append_%s%s%s%skernel<%d,%s>", c.varlen ? "varlen_" : "paged_", c.pos ? "pos_" : "", c.a.kv_bytes == 1 ? "kv8_" : "",
           c.bf16 ? "bf16_" : "", c.a.D, c.flags & LC_ROPE_INTERLEAVED ? "true" : "false");
}

// The name of what an attention plan launches (lc_attn_kernel_name_bh / _ex; bench.py, tools/ and the tests parse these strings).
void format_attn(const AttnPlan& p, char* buf, int buflen) {
  const int D = p.call.D;
  const bool v_transposed = p.call.vt;
  const char* vt = v_transposed ? "true" : "false";
  const char* bf = p.call.bf16 ? "true" : "false";
  switch (p.kern) {
    // (a persistent walk with no more blocks than CUs launches WALK 0; the name reports the walk asked for at this N; 3 = split-KV, whose
    // launch also runs attn_split_combine_kernel<D>)
    case AKern::W4U: snprintf(buf, buflen, "attn_fwd_w4u_kernel<%d,%s,%d>", D, vt, p.walk); break;
    case AKern::W4I: snprintf(buf, buflen, "attn_fwd_w4i_kernel<%d,%d>", D, p.sched); break;
    case AKern::LOCKSTEP: snprintf(buf, buflen, "attn_fwd_kernel<%d,%d,%s,0>", D, p.nw, vt); break;
    case AKern::BIGD4: snprintf(buf, buflen, "attn_fwd_bigd4_kernel<%d>", p.span8 == 0 ? 8 : p.span8); break;
    case AKern::BIGD6: snprintf(buf, buflen, "attn_fwd_bigd6_kernel<%s>", bf); break;
    case AKern::BIGD7: snprintf(buf, buflen, "attn_fwd_bigd7_kernel<%s,%s>", bf, vt); break;
    case AKern::BIGD2: snprintf(buf, buflen, "attn_fwd_bigd2_kernel<%d,%s,%s>", D, v_transposed ? "false" : bf, vt); break;   // (V transposed: fp16 only)
    case AKern::BIGD3: snprintf(buf, buflen, "attn_fwd_bigd3_kernel<%d,%s>", D, bf); break;
    case AKern::COLSPLIT: snprintf(buf, buflen, "attn_fwd_bigd_kernel<%d,%d,%d,%s,%s>", D, D > 256 ? 256 : D, p.nw, vt, bf); break;
    case AKern::W4U_CAUSAL: snprintf(buf, buflen, "attn_fwd_w4u_causal_kernel<%d,%s>", D, vt); break;
    case AKern::LOCKSTEP_CAUSAL: snprintf(buf, buflen, "attn_fwd_causal_kernel<%d,%d,%s>", D, p.nw, vt); break;
  }
  if (p.call.gqa > 1) {   // the grouped-query twin: "_kernel<" -> "_gqa_kernel<", same template arguments
    char* at = strstr(buf, "_kernel<");
    const size_t len = strlen(buf);
    if (at && len + 4 < (size_t)buflen) {
      memmove(at + 4, at, len - (size_t)(at - buf) + 1);
      memcpy(at, "_gqa", 4);
    }
  }
}

}  // namespace lc
