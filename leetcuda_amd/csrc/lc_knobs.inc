// lc_knobs.inc — THE list of run-time tuning knobs (lc_tune_set / lc_tune_get): experiments and A/B benches, never required for correctness.
// One row per knob, in the order lc_tune_key reports them:
//     LC_KNOB(name, default, validator, diagnosis-only)        steers only the inside of a kernel: read by its launcher
//     LC_KNOB_SNAP(name, default, validator, diagnosis-only)   decides which kernel runs: a field of the per-call snapshot `Knobs`
// The including site defines LC_KNOB (and LC_KNOB_SNAP where the two differ) and gets both undefined again.  The storage
// (tune_t g_tune_<name>), its default, the snapshot field and its by-name fill (read_knobs) and the registry row (kKnobs, key = #name) all
// come from the row: lc_plan.h, tu_plan.hip.  A diagnosis-only key (include/lc_diag.h) may give WRONG results; a production library rejects it.
#ifndef LC_KNOB_SNAP
#define LC_KNOB_SNAP LC_KNOB
#endif
LC_KNOB_SNAP(attn_nw, 0, ok_attn_nw, false)               // attention kernel for D <= 128: 0 = auto, 513 / 515 / 517 / 514 / 8 / 4 / 2 (choose_attn_nw, lc_abi.h)
LC_KNOB_SNAP(attn_walk, 0, ok_03, false)                  // block walk of the merged-phase kernel under attn_nw = 0: 0 = auto by N, 1 / 2 / 3 = WALK 0 / 1 / 2
LC_KNOB_SNAP(attn_split, 0, ok_split, false)              // split-KV of the merged-phase kernel on grids that do not fill the GPU: 0 = auto (attn_split_auto), 1 = off, 2 / 4 / 8 / 16 = that many KV ranges per query block
LC_KNOB_SNAP(attn_decode_split, 0, ok_064, false)          // KV ranges per (batch, K / V head) of the decode kernel (attn_decode.hip): 0 = auto (plan_attn_decode), 1 .. 64 = exactly that many (empty ranges are legal)
LC_KNOB_SNAP(attn_causal_order, 0, ok_02, false)          // grid order of the causal merged-phase kernel: 0 = auto (choose_attn_causal), 1 = longest query block first, 2 = head-major (xcd_remap; same bits)
LC_KNOB(attn_bigd_map, 0, ok_02, false)                   // block -> query block map of attn_bigd4 / attn_bigd6: 0 = auto (D = 1024: round-robin over the XCDs, D = 512: XCD-contiguous), 1 = XCD-contiguous, 2 = round-robin (same bits; profiles/r5f_bigd_map.log)
LC_KNOB(attn_bigd_stagger, 0, ok_02, false)               // attn_bigd4 (D = 1024): the KV walk of the workgroups on XCD x starts x eighths of the sequence in: 0 = auto (with the round-robin block map), 1 = off, 2 = on (results agree to rounding)
LC_KNOB_SNAP(attn_d1024, 0, ok_span8, false)              // attn_bigd4's DMA spread in eighths of a phase: 0 = default (8), 2 / 4 / 6 (A/B knob)
LC_KNOB_SNAP(attn_w4i_sched, 1, ok_01, false)             // schedule of attn_fwd_w4i_kernel's generated phase statements (tools/gen_attn_w4i.py NSCHED; same bits)
LC_KNOB_SNAP(fp8_mx, 3, ok_03, false)                     // fp8 GEMM (plan_gemm_fp8): 3 = MX K=128 MFMA, generated loop (gemm_fp8_w4k.hip); 1 = MX K=64, 4-wave kernel; 2 = MX K=64, 8-wave kernel; 0 = plain K=16 MFMA
LC_KNOB_SNAP(attn_d512, 0, ok_04, false)                  // D = 256 / 512 / 1024: 0 = auto, 1 = column-split kernel, 2 = attn_bigd3, 3 = D = 256 / 512 on the other MFMA shape than auto (attn_bigd2 <-> attn_bigd7 / attn_bigd6), 4 = auto but attn_bigd7 on any grid
LC_KNOB_SNAP(w4y_sched, 2, ok_w4y_sched, false)           // hgemm_w4y_kernel loop schedule 0..2 (lc_tune_set "w4y_sched"; same bits; 0 / 1: k-step outer; 2 (default): the pair loop, hgemm_w4y_loop_pair.inc — both k-steps of an accumulator block back to back, the DMA pieces spread evenly — fewer joules per MFMA at the power cap, profiles/mfma_pair_probe.log, profiles/hgemm_pair_ab.log)
LC_KNOB(hgemm_persist, 1, ok_01, false)                   // 1 (default) = hgemm_w4y_kernel as a persistent workgroup per CU when the tiles divide evenly (lc_tune_set "hgemm_persist")
LC_KNOB(hgemm_stagger, 0, ok_stagger, false)              // K-loop stagger of hgemm_w4y_kernel (lc_tune_set "hgemm_stagger"): 0 = auto (by XCD), 1 << 27 = off, else cx | cm << 4 | cn << 8 | step << 12 | mask << 20
LC_KNOB_SNAP(hgemm_tail, 1, ok_04, false)                 // 1 = hand the ragged last wave of the 256-tile kernel to 128 x 128 blocks (launch_mfma256: the mid-size kernel; 2 = round 5's 128-tile kernel + split-K), 0 = one launch
LC_KNOB_SNAP(hgemm_tail_tile, 0, ok_02, false)            // sub-tiles of the ragged tail on the mid-size kernel: 0 = auto (launch_mfma256), 1 = 64 x 128 eighths, 2 = 128 x 128 quadrants
LC_KNOB_SNAP(hgemm_ragged, 0, ok_01, false)               // LC_HGEMM_AUTO on ragged M / N with K % 32 == 0: 0 = LC_HGEMM_RAGGED (the tiled kernels, clamped 128 x 128 tiles on what they do not divide), 1 = never (hgemm_edge_kernel)
LC_KNOB_SNAP(hgemm_ragged_fork, 0, ok_02, false)          // LC_HGEMM_RAGGED's border launch on a side stream, forked from and joined to the caller's (runs beside the interior): 0 = auto (launch_ragged), 1 = never, 2 = always
LC_KNOB_SNAP(hgemm_ragged_tile, 0, ok_ragged_tile, false) // tile of a ragged problem that runs entirely on hgemm_mid_edge_kernel: 0 = auto (ragged_plan), 12 / 22 / 23 / 32 / 33 = that tile (rows / 64, columns / 64; A/B)
LC_KNOB_SNAP(hgemm_kpad, 0, ok_02, false)                 // LC_HGEMM_AUTO on K % 32 != 0 (K % 8 == 0): 0 = auto (zero-padded operand copies + the tuned kernels from a quarter of a 128 x 128 block per CU on), 1 = never (hgemm_edge_kernel), 2 = wherever legal
LC_KNOB_SNAP(hgemm_mid_splitk, 0, ok_08, false)           // split-K of the mid-size kernel: 0 = auto (mid_tile_auto), 1 = never, 2 .. 8 = that many K ranges wherever legal (A/B)
LC_KNOB_SNAP(hgemm_128w, 0, ok_02, false)                 // waves of the 128-tile kernel: 0 = auto (eight — intra-workgroup split-K — on grids of <= 0.6 blocks per CU), 1 = always four, 2 = always eight
LC_KNOB_SNAP(rule_cus, 0, ok_rule_cus, false)             // CU count the LAUNCH RULES reason with: 0 = the current device's own; 64 .. 1024 = that many (tests of the rules for other devices; grids are always sized with the real count)
LC_KNOB_SNAP(attn_calib, 0, ok_01, false)                 // split-KV cost model: 0 = the constants lc_tune_calibrate measured on this device when it ran (else the built-in ones), 1 = always the built-in ones
LC_KNOB_SNAP(hgemm_mid, 0, ok_mid, false)                 // mid-size kernel (hgemm_mid.hip): 0 = auto (mid_tile_auto), 1 = never, 12 / 13 / 22 / 23 / 32 / 33 = that tile (rows / 64, columns / 64)
LC_KNOB_SNAP(hgemm_mid_ns, 0, ok_mid_ns, false)           // ... its LDS ring slots: 0 = auto (3 for one-round grids, else 2), 2, 3
LC_KNOB_SNAP(hgemm_splitk, 0, ok_08, false)               // split-K of the 128-tile blocks that serve border strips / the ragged last wave: 0 = auto (launch_mfma256), 1 = off, 2 .. 8 = that factor
LC_KNOB_SNAP(hgemm_raster, 0, ok_02, false)               // block -> C tile map: 0 = auto (by operand footprint, panel_tiles), 1 = the reference's block swizzle (N panels from
                                                          // swizzle_stride, XCD-contiguous ids), 2 = XCD super-block raster (hgemm_mfma256.hip raster_xcd16)
LC_KNOB_SNAP(hgemm_auto, LC_HGEMM_MFMA256W4Y, ok_auto, false)   // what LC_HGEMM_AUTO launches for large 256-tileable shapes (lc_tune_set "hgemm_auto")
LC_KNOB_SNAP(w4_abl, 0, ok_any, true)                     // hgemm_w4 ablation bits (diagnosis only, LC_DIAG)
LC_KNOB_SNAP(hgemm_stamps, 0, ok_01, true)                // GEMM cycle-stamp builds (diagnosis only, LC_DIAG)
LC_KNOB_SNAP(attn_ablate, 0, ok_any, true)                // attention ablation / stamp builds (diagnosis only, LC_DIAG)
#undef LC_KNOB
#undef LC_KNOB_SNAP
