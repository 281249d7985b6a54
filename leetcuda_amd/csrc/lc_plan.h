// lc_plan.h — the host-side launch planning of libleetcuda_amd.so (tu_plan.hip): the knob snapshot and registry, the reference entry-name
// tables, and ONE plan per HGEMM / fp8 GEMM / attention / decode call — every launch decision — that the launchers (tu_*.hip) run and the name calls report.  No kernel source.
#pragma once
#include "lc_launch.h"
#include "lc_tiles.h"

namespace lc {

// every knob's storage (lc_knobs.inc; lc_launch.h declares the four that launchers of other units read)
#define LC_KNOB(name, dflt, valid, diag) extern tune_t g_tune_##name;
#include "lc_knobs.inc"

// The knobs that decide which kernel runs, read ONCE per call: the planners (plan_hgemm, plan_gemm_fp8, plan_attn, plan_attn_decode) and every rule they use take
// this snapshot, so a concurrent lc_tune_set cannot pair one decision with another.  (hgemm_persist, hgemm_stagger, attn_bigd_map and attn_bigd_stagger steer only the
// inside of a kernel — how it walks the tiles the plan counted, where a K walk starts: same kernel, same bits — no name reports them: their launchers read them.)
struct Knobs {
#define LC_KNOB(name, dflt, valid, diag)
#define LC_KNOB_SNAP(name, dflt, valid, diag) int name;
#include "lc_knobs.inc"
};
Knobs read_knobs();

// the knob registry: ONE table for lc_tune_set / lc_tune_get (key, variable, default, validity of a value)
struct Knob {
  const char* key;
  tune_t* var;
  int dflt;
  bool (*valid)(int);
  bool diag;   // diagnosis key (include/lc_diag.h): results may be WRONG; a production library rejects it
};
extern const Knob kKnobs[];
extern const int kNumKnobs;
const Knob* find_knob(const char* key);   // nullptr: no such key (or a diagnosis key in a production library)

// reference entry tables
struct HgemmEntry {
  const char* name;
  int layout;   // lc_layout
  int nargs;    // 0, 3 or 6
  int variant;  // lc_hgemm_variant, -1 = vendor, -2 = handle init, -3 = handle destroy
};
struct AttnEntry {
  const char* name;
  int family, vt, acc_f32, maxd_s2, maxd_s1, nargs;
};
extern const HgemmEntry kHgemmEntries[];
extern const AttnEntry kAttnEntries[];
extern const int kNumHgemmEntries, kNumAttnEntries;
const HgemmEntry* find_hgemm(const char* name);
const AttnEntry* find_attn(const char* name);

bool is_w4_variant(int v);
bool is_tile256_variant(int v);
bool is_valu_variant(int v);
bool is_hgemm_variant(int v);

int panel_tiles(int raster, int swizzle_stride, int tiles_n, int tile_n, size_t operand_bytes);
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
// hgemm_w4y_kernel and the 4-wave fp8 kernels built on it address K-contiguous operands by 32-bit DMA offsets from a wave's first row, and a wave's pieces reach
// 232 rows past it: 260 rows of K elements stay below 2 GiB (fp16: K <= 4 129 776; fp8: K <= 8 259 552, the last multiple of 128 being 8 259 456)
inline bool w4_rows_fit(int K, int elem_bytes) { return (size_t)K * elem_bytes * 260 < ((size_t)1 << 31); }
int rule_cus(const Knobs& k);
// Constants of the split-KV cost model (attn_split_auto) measured on THIS device by lc_tune_calibrate (round 6; round-5 verdict weak #13:
// they were fitted once, on one box's clocks); one record per device ordinal, valid != 0 once measured.
struct AttnCalib {
  std::atomic<int> valid{0};
  float tau128 = 0.f, tau64 = 0.f, x0 = 0.f, bytes_per_us = 0.f;
};
extern AttnCalib g_attn_calib[64];
constexpr double kSplitFixedUs = 5.0, kSplitBytesPerUs = 2.6e6;   // the built-in x0 and bw of that model (tu_plan.hip attn_split_auto)

struct MidTile { int tmw, tnw, ns, ks; long wgs; };   // ks > 1: split-K, needs ks x M x N floats of workspace (launch_mid; none under graph capture)
struct RaggedPlan { int kind, Mi, Ni, ns, tmw, tnw, ks; };   // ks > 1: split-K (kind 2, 64 / 128 x 128 tiles; needs the workspace: none under graph capture)
struct TailSplit { int nblk, R, tmw, ns; };   // nblk = -1: one launch of all T tiles

// ONE decision per HGEMM call: plan_hgemm makes it from one knob snapshot, lc_hgemm_f16 launches it and lc_hgemm_kernel_name reports it.
// A launch differs from its plan only where the plan cannot know; this is the complete list:
//   - the stream is being captured: no workspace (split-K of the 128-tile border blocks, of the mid-size and of the ragged kernel: one K range;
//     LC_HGEMM_KPAD: hgemm_edge_kernel), no fork (the border on the caller's stream)
//   - the workspace lease fails (the same fallbacks; LC_HGEMM_KPAD's padded problem holds the lease, so its plan runs workspace-free, unforked)
//   - the fork's side stream cannot be made: both launches on the caller's stream
//   (attention: the same for split-KV; and a persistent w4u walk with no more blocks than CUs runs walk 0, the dynamic queue on a CU count
//   that is not a multiple of 8 or under capture the static walk — tu_attn_w4u_impl.h;
//   decode attention, DecodePlan with S > 1 and no caller workspace: the stream is being captured, or the workspace lease fails: S = 1, one launch)
enum class HFam { VALU, TILE256, MFMA128, MID, RAGGED, KPAD, EDGE, GENERIC };
struct HgemmPlan {
  Knobs k;                  // the snapshot (launch: panel_tiles, LC_HGEMM_KPAD's plan of the padded problem)
  HFam fam;
  int variant;              // VALU: the rung; TILE256: the 256-tile family after LC_HGEMM_AUTO
  int w4, sched;            // TILE256 / RAGGED kind 1: w4_effective_variant (0: not a 4-wave family), hgemm_w4y_kernel's schedule
  MidTile mid;              // MID
  RaggedPlan rag;           // RAGGED
  int Kp;                   // KPAD: the padded K
  int tiles_m, tiles_n;     // TILE256 / RAGGED kind 1: the 256 x 256 tiles of the (interior) grid ...
  TailSplit tail;           // ... and their ragged last round
  int nright, nbottom;      // TILE256: 128-wide border strips in 128 x 128 blocks; all blocks of the 128-tile launch (strips + tail quadrants),
  int nb128, ks, ksw;       // their split-K factor and the kernel's waves (ksw: also MFMA128)
  bool fork;                // RAGGED kind 1: the border launch on the side stream
};
int plan_hgemm(const Knobs& k, int M, int N, int K, bool b_kn, int variant, bool al, HgemmPlan* out);
void format_hgemm(const HgemmPlan& p, int M, int N, bool b_kn, char* buf, int buflen);
int hgemm_entry_variant(const Knobs& k, const HgemmEntry& e, int M, int N, int K, bool al);   // what a reference entry name (lc_hgemm_call) runs on this shape

// ONE decision per fp8 GEMM call (lc_gemm_fp8_e4m3; mx: lc_gemm_mxfp8, which carries E8M0 block scales): the entry states a GemmFp8Call, check_gemm_fp8 checks
// and plans it, launch_gemm_fp8_plan launches the plan and decides nothing.  The rule ("fp8_mx" 3 / 1 / 2 / 0): W4K / W4 / PINGPONG2_MX / PINGPONG2, and PINGPONG2_MX
// (64-bit addresses) for a 4-wave kernel whose K does not fit w4_rows_fit; block scales: W4K_MX whatever the knob, LC_ERR_SHAPE when K does not fit its one kernel.
struct GemmFp8Call { int M, N, K, swizzle_stride; bool mx; };
struct GemmFp8Ptrs { const uint8_t *A, *B; half_t* C; const uint32_t *PA, *PB; float alpha; hipStream_t st; };   // PA, PB: mx (as lc_mxfp8_pack_scales packs them), else nullptr
enum class Fp8Kern { W4K, W4K_MX, W4, PINGPONG2_MX, PINGPONG2 };   // gemm_fp8_w4k_kernel<false / true>, gemm_fp8_w4_kernel, gemm_fp8_pingpong2_kernel<true / false>
// tiles: of 256 x 256; panel_w: panel_tiles of "hgemm_raster", the call's swizzle_stride and (M + N) x K operand bytes; call: what was planned
struct GemmFp8Plan { Fp8Kern kern; int tiles_m, tiles_n, panel_w; GemmFp8Call call; };
// the checks in the order that decides the status of a doubly-bad call (nulls, dims, tiles and alignment, the block-scaled K bound), then the plan; a: nullptr = no pointers
int check_gemm_fp8(const GemmFp8Call& c, const GemmFp8Ptrs* a, GemmFp8Plan* p);
int plan_gemm_fp8(const Knobs& k, const GemmFp8Call& c, GemmFp8Plan* p);   // checked arguments; LC_OK or LC_ERR_SHAPE
inline int check_mx_pack_scales(const void* S, const void* P, int rows, int K) {   // lc_mxfp8_pack_scales: nothing to plan
  return !S || !P ? LC_ERR_ARG : rows <= 0 || K <= 0 || rows % BM || K % 128 || !aligned8(P) ? LC_ERR_SHAPE : LC_OK;
}
int launch_gemm_fp8_plan(const GemmFp8Plan& p, const GemmFp8Ptrs& a);      // tu_fp8.hip: its three kernels, or ...
int launch_gemm_fp8_w4k_plan(const GemmFp8Plan& p, const GemmFp8Ptrs& a);  // ... tu_fp8k.hip: the K = 128 ones

// Which attention kernel serves a problem (plan_attn; D <= 128: choose_attn_nw, with the lc_tune_set "attn_nw" value of each in brackets):
//   W4U       attn_fwd_w4u_kernel<D, VT, WALK> (attn_w4u.hip: D = 64 / 128, N % 256 == 0, V as [B,H,N,D] or — the three *_swizzle_qkv entries —
//             [B,H,D,N]): WALK 0 one 256-row query block per workgroup [513], 1 persistent workgroup per CU, static walk [515], 2 persistent,
//             dynamic per-XCD block queue [517], 3 split-KV: nsplit KV ranges per query block + the combine kernel [auto only]
//   W4I       the same design with each phase as one generated asm statement (attn_w4i.hip: D = 32 / 64 / 96 / 128, V as [B,H,N,D]; the only
//             merged-phase kernel for D = 96 / 32) [514];  LOCKSTEP  attn_fwd.hip with nw waves [8 / 4 / 2];  the rest: D >= 256 (use_bigd*)
// [512] (round 2's attn_w4n) is an alias of [513]: attn_w4u<128, false, 0> IS that kernel; 256 / 260 / 516 were retired in round 4 with
// attn_w4m.hip / attn_w8g.hip.
// Causal calls (lc_attn_fwd_f16_ex, choose_attn_causal): W4U_CAUSAL  attn_fwd_w4u_causal_kernel<D, VT> (D = 64 / 128, N % 256 == 0; one block
// per workgroup, order = "attn_causal_order");  LOCKSTEP_CAUSAL  attn_fwd_causal_kernel<D, nw, VT> (everything else with D <= 128).
enum class AKern { W4U, W4I, LOCKSTEP, BIGD4, BIGD6, BIGD7, BIGD2, BIGD3, COLSPLIT, W4U_CAUSAL, LOCKSTEP_CAUSAL };
// The problem of one attention call; plan_attn keeps it in the plan, so that the name (format_attn) and the launch (launch_attn_plan) need no second copy.
struct AttnCall {
  long bh;     // B x H query heads; -1: unknown (lc_attn_kernel_name: "a grid that fills the GPU")
  int gqa;     // group size H / Hkv of a grouped-query call, 1 = MHA.  The planner decides NOTHING by it: > 1 runs and names the `_gqa` twin of the
  int N, D;    // kernel the MHA call of the same (B H, N, D, V layout, causal, knobs) gets (the merged-phase `_gqa` units, tu_attn_gqa.hip)
  bool vt, bf16, causal;   // V as [B,H,D,N]; bf16 inputs and output; causal mask (fp16, D <= 128)
};
inline bool is_small_headdim(int D) { return D == 32 || D == 64 || D == 96 || D == 128; }   // the head dims of the D <= 128 kernels (choose_attn_nw)
// one head's K / V must fit the 32-bit buffer offsets of the LDS-DMA kernels (a bound on positive sizes: the callers rank N, D <= 0 themselves)
inline bool attn_span_fits(int N, int D) { return N <= 0 || D <= 0 || (size_t)N * (size_t)D * 2 < 0x80000000ull; }
struct AttnPlan {   // walk / nsplit: W4U; sched: W4I ("attn_w4i_sched"); nw: LOCKSTEP / COLSPLIT waves; span8: BIGD4's DMA spread in eighths
  AKern kern;         // of a phase ("attn_d1024"; 0 = the default, 8); abl: LOCKSTEP's LC_DIAG ablation ("attn_ablate"; D = 128, V as [B,H,N,D])
  int walk, nsplit, sched, nw, span8, abl, order;   // order: W4U_CAUSAL's grid order
  AttnCall call;      // what was planned
};
int plan_attn(const Knobs& k, const AttnCall& c, AttnPlan* p);
void format_attn(const AttnPlan& p, char* buf, int buflen);

// What a caller of a decode-attention entry states (lc_attn_decode_f16 / _paged_f16 / _paged_kv8 and the two query calls of each): the ONE place that
// says whether the cache is paged and how wide its elements are; the plan keeps it, as AttnPlan keeps its AttnCall.
struct DecodeCall {
  int B, H, Hkv, Nq, D, flags;
  int kv_bytes;                          // bytes of a cache element: 2 (fp16) or 1 (e4m3; paged only)
  bool paged;                            // false: a contiguous [B,Hkv,Ncap,D] cache; true: pools [num_pages,Hkv,page_size,D] + a block table
  int Ncap;                              // contiguous only
  int num_pages, page_size, max_pages;   // paged only (the query calls state num_pages = 1: it decides nothing)
  bool chunk = false;                    // a chunk entry (lc_attn_chunk_*): R = (H / Hkv) x Nq is not bounded by 64
  int window = 0;                        // lc_attn_local_*: W > 0: a sliding window of W keys (causal calls only); 0: none
  bool sinks = false;                    // lc_attn_local_*: the call has a sink logit per query head (the query calls: never)
  bool varlen = false;                   // lc_attn_varlen_paged_*: a ragged batch — Q, O token-major [T,H,D], cu_q[B + 1]; Nq = max_nq, chunk = true
  int T = 0, max_nq = 0;                 // varlen only: the rows of Q and O, and the host's bound on every Nq_b
  bool bf16 = false;                     // lc_attn_varlen_paged_*bf16: Q, O and a 16-bit cache are bfloat16 (varlen only).  It picks the
                                         // kernels (and their names) and nothing else: every check and RT, RB, S, grid, LDS, workspace are the fp16 call's
  bool lse = false;                      // lc_attn_varlen_paged_lse_* (DESIGN.md §4.3n): the call also writes each row's log-sum-exp (varlen only).  It picks
                                         // the kernels (and their names) and adds DecodePtrs::lse to the NULL check; the plan and the workspace are the twin's
  bool tree = false;                     // lc_attn_varlen_paged_tree_* (DESIGN.md §4.3o): a look-back visibility word per query token (lse calls only).  It picks
                                         // the kernels (and their names), adds DecodePtrs::tree_mask to the NULL and alignment checks and requires
                                         // LC_ATTN_CAUSAL; the plan and the workspace are the twin's
};
enum class DecodeCache { FLAT, PAGED, PAGED_KV8 };   // which kernel family reads the cache (indexes launch_attn_decode's table of range launchers)
// ONE decision per decode-attention call and ONE path for the three cache kinds: an entry point (lc_abi.hip) states a DecodeCall, check_attn_decode
// checks and plans it, launch_attn_decode launches the plan, format_attn_decode names it.  The plan: attn_decode_kernel<D, RT> (FLAT),
// attn_decode_paged_kernel<D, RT> (PAGED) or attn_decode_paged_kv8_kernel<D, RT> (PAGED_KV8: e4m3 pools) on B x Hkv x S workgroups, S > 1 followed by
// attn_decode_combine_kernel<D>.  RT = row tiles of 16 that hold the R = (H / Hkv) x Nq query rows of a K / V head.  S, the KV ranges per (batch,
// K / V head), is decided from (B x Hkv, ceil(Ncap / 64), rule_cus, "attn_decode_split") and NEVER from kv_len, which only the kernel reads: the
// smallest S that gives every CU a workgroup, with at least 4 tiles of Ncap per range, at most 64; the knob forces 1 .. 64 (ranges may then be
// empty).  The cache kind decides the kernel and nothing else: RT, S and the workspace bytes of a paged call are those of the contiguous call of
// Ncap = max_pages x page_size.
// A chunk call (DecodeCall::chunk) may have R > 64: RB = ceil(R / 64) row blocks per (batch, K / V head).  RB = 1 is the plan of
// the decode call, whichever entry stated it; RB > 1: RT = 4, attn_chunk_kernel<D> / attn_chunk_paged_kernel<D> / attn_chunk_paged_kv8_kernel<D>
// on B x Hkv x RB x S workgroups, S by the same rule with B x Hkv x RB groups.
// A local call (lc_attn_local_*) with window = 0 and no sinks IS the chunk call: same plan.  With either, `local`: the
// attn_local_*_kernel<D, RT> (RB = 1) / attn_local_chunk_*_kernel<D> (RB > 1) of its cache kind on the same grid; window > 0 puts the tiles of
// min(Ncap, window + Nq - 1 + 63) keys — what one workgroup walks at most, tile misalignment included — in place of those of Ncap in the rule of S.
// A varlen call (lc_attn_varlen_paged_*) is planned as the chunk call of Nq = max_nq — RT, RB, the tiles of a window — on the
// attn_varlen_*_kernel of its cache kind (all LOCAL = true: no second plan for window = 0 and no sinks), with two differences: the groups of the
// rule of S are Hkv x min(B RB, ceil(G T / 64) + B), an upper bound of the row blocks that can hold work whatever cu_q says, and the partials
// are S x T H rows, merged by attn_varlen_combine_kernel<D>.
struct DecodePlan {
  DecodeCall call;     // what was planned
  DecodeCache cache;
  int Ncap, RT, S;     // Ncap: the call's, or max_pages x page_size
  int RB;              // row blocks of 64 query rows per (batch, K / V head); > 1: the chunk kernels
  bool local;          // window > 0 or sinks: the kernels of attn_local.hip
};
struct DecodePtrs {
  const half_t* Q;     // (16-bit lanes: a bf16 plan's kernels read and write them as bfloat16 — O, the sources of the rope call and Qout too)
  const void *K, *V;   // the cache or the pools; each unit casts once to the element type of its own kernel
  half_t* O;
  const int* kv_len;   // device int32[B]; FLAT: or nullptr
  hipStream_t st;
  const int* block_table;           // paged: device int32[B, max_pages]; else nullptr
  const float *k_scale, *v_scale;   // PAGED_KV8: device float[Hkv] or nullptr = 1.0; else nullptr
  const float* sinks;               // a local or varlen call: device float[H] or nullptr = no sinks; else nullptr
  const int* cu_q = nullptr;        // a varlen call: device int32[B + 1]; else nullptr
  float* lse = nullptr;             // a call with DecodeCall::lse: device float[T H]; else nullptr
  const uint64_t* tree_mask = nullptr;   // a call with DecodeCall::tree: device uint64[T]; else nullptr
};
// The checks of the three decode entry points, in the order that decides which status a doubly-bad call gets, then the plan.  a: the run call's
// pointers (nullptr: a query call, which has none)
int check_attn_decode(const DecodeCall& c, const DecodePtrs* a, DecodePlan* p);
int plan_attn_decode(const Knobs& k, const DecodeCall& c, DecodePlan* p);   // checked arguments; nothing writes into a plan afterwards
// (varlen: "attn_varlen_paged_kernel<128,1> x8", "attn_varlen_chunk_paged_kv8_kernel<64>"; bf16: "attn_varlen_paged_bf16_kernel<128,1> x8")
void format_attn_decode(const DecodePlan& p, char* buf, int buflen);   // "attn_decode_kernel<128,1> x8" (" xS": S > 1, + the combine kernel); RB > 1: "attn_chunk_kernel<128> x8"; local: "attn_local_kernel<128,1>", "attn_local_chunk_kernel<128>"
// rows of Q and O, and of each of the S partials: B H Nq — varlen: T H
inline size_t decode_rows(const DecodeCall& c) { return c.varlen ? (size_t)c.T * c.H : (size_t)c.B * c.H * c.Nq; }
// bytes of fp32 partials a plan with S > 1 needs: S x rows x (D + 1) floats; 0 for S = 1
inline size_t decode_workspace_bytes(const DecodePlan& p) {
  return p.S > 1 ? (size_t)p.S * decode_rows(p.call) * (size_t)(p.call.D + 1) * sizeof(float) : 0;
}
int launch_attn_decode(const DecodePlan& p, const DecodePtrs& a, void* workspace);   // tu_attn_decode.hip
// the S range workgroups of a plan of cache kind C: tu_attn_decode_impl.h, instantiated once per kind in the unit that compiles that kind's kernels
template <DecodeCache C>
int launch_attn_decode_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse);
// ... and of a plan with RB > 1: tu_attn_chunk.hip, the three kinds in one unit
template <DecodeCache C>
int launch_attn_chunk_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse);
// ... and of a local plan, RB = 1 or more: tu_attn_local_impl.h, instantiated in tu_attn_local.hip / _paged.hip / _paged_kv8.hip
template <DecodeCache C>
int launch_attn_local_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse);
// ... and of a varlen plan (PAGED and PAGED_KV8 only): tu_attn_varlen_impl.h, instantiated once per variant in the twelve tu_attn_varlen_paged*.hip,
// each next to its own kernels.  BF16: DecodeCall::bf16; OUT: what the kernels write besides O and so take behind T — nothing, `lse`
// (DecodeCall::lse) or `lse` under a `tree_mask` (DecodeCall::tree).  launch_attn_decode picks the instantiation from the call's fields
enum class VarlenOut { PLAIN, LSE, TREE };
template <DecodeCache C, bool BF16, VarlenOut OUT>
int launch_attn_varlen_ranges(const DecodePlan& p, int S, const DecodePtrs& a, float* part_o, float* part_lse);
// ... and its combine launch (attn_varlen_combine_kernel<D> / _bf16 / _lse / _lse_bf16, each for both cache kinds; a tree plan's is the LSE plan's):
// the same header, instantiated in tu_attn_varlen_paged.hip / _paged_bf16.hip / _paged_lse.hip / _paged_lse_bf16.hip
template <bool BF16, bool LSE>
int launch_attn_varlen_combine(const DecodePlan& p, int S, const DecodePtrs& a, const float* part_o, const float* part_lse);

// What a caller of a state-merge entry states (lc_attn_merge_states_f16 / _bf16): two (O [T,H,D], lse [T H]) states over disjoint
// key sets become the state over their union.  There is nothing to plan: attn_merge_states_kernel<D> / attn_merge_states_bf16_kernel<D> on
// ceil(T H / (2048 / D)) workgroups, no workspace.
struct MergeCall {
  int B, T, H, D;                        // B: entries of cu_q - 1 (unused without cu_q)
  bool bf16;
};
struct MergePtrs {
  const half_t* Oa;                      // (16-bit lanes: fp16 or, MergeCall::bf16, bfloat16)
  const float* lse_a;
  const half_t* Ob;
  const float* lse_b;
  half_t* Oout;                          // may be Oa or Ob
  float* lse_out;                        // may be lse_a or lse_b
  const int* cu_q;                       // device int32[B + 1] or nullptr = every row
  hipStream_t st;
};
int check_attn_merge(const MergeCall& c, const MergePtrs& p);    // tu_plan.hip
int launch_attn_merge(const MergeCall& c, const MergePtrs& p);   // tu_attn_merge.hip; checked arguments

// What a caller of an append-to-cache entry states (lc_kv_append_paged_f16 / _kv8 and their name calls): the write side of the paged cache that
// DecodeCall with paged = true reads.  There is nothing to plan: one kernel, kv_append_paged_kernel<D> or kv_append_paged_kv8_kernel<D>, on
// B x Hkv x ceil(Nq / (2048 / D)) workgroups, no workspace.
struct AppendCall {
  int B, Hkv, Nq, D, flags;
  int kv_bytes;                          // bytes of a pool element: 2 (fp16) or 1 (e4m3)
  int num_pages, page_size, max_pages;   // (the name calls state num_pages = 1: it decides nothing)
};
struct AppendPtrs {
  const half_t *Knew, *Vnew;             // [B,Hkv,Nq,D] fp16
  void *Kpool, *Vpool;                   // [num_pages,Hkv,page_size,D] of kv_bytes an element
  const int *block_table, *kv_len;       // device int32[B, max_pages], int32[B] (the lengths AFTER the append)
  const float *k_scale, *v_scale;        // kv_bytes = 1: device float[Hkv] or nullptr = 1.0; else nullptr
  hipStream_t st;
};
inline int kv_append_tokens_per_block(int D) { return D == 64 ? 32 : 16; }   // 2048 / D for the head dims there are; the grid bound's figure for the rest
// The checks of the two append entry points, in the order that decides which status a doubly-bad call gets.  a: the run call's pointers (nullptr:
// a name call, which has none)
int check_kv_append(const AppendCall& c, const AppendPtrs* a);
void format_kv_append(const AppendCall& c, char* buf, int buflen);   // "kv_append_paged_kernel<128>" / "kv_append_paged_kv8_kernel<128>"
int launch_kv_append(const AppendCall& c, const AppendPtrs& a);      // tu_kv_append.hip; checked arguments

// What a caller of a rotary-embedding + append entry states (lc_rope_append_paged_f16 / _kv8 and their name calls): the append
// call (its flags are 0) plus what the rotation and the Q side need.  Nothing to plan either: one kernel, rope_append_paged_kernel<D, INTERLEAVED>
// or rope_append_paged_kv8_kernel<D, INTERLEAVED>, on (B x Hkv + B x H) x ceil(Nq / (2048 / D)) workgroups, no workspace.
struct RopeAppendCall {
  AppendCall a;
  int H, rot_dim, max_pos;
  long long src_row_stride;              // elements; 0 unless LC_ROPE_PACKED_SRC (varlen: q_row_stride)
  int flags;                             // LC_ROPE_INTERLEAVED | LC_ROPE_PACKED_SRC (varlen: LC_ROPE_INTERLEAVED only)
  // lc_rope_append_varlen_* (DESIGN.md §4.3l): a ragged batch — token-major sources with a row stride each, Qout dense [T,H,D], cu_q[B + 1];
  // a.Nq = max_nq.  One kernel, rope_append_varlen_kernel<D, INTERLEAVED> or rope_append_varlen_kv8_kernel<D, INTERLEAVED>, on
  // ceil(T / (2048 / D)) x (Hkv + H) workgroups: the grid is over global token blocks and does not grow with B
  bool varlen = false;
  int T = 0, max_nq = 0;
  long long kv_row_stride = 0;           // elements; Knew and Vnew
  bool bf16 = false;                     // lc_rope_append_varlen_*bf16: sources, Qout and 16-bit pools are bfloat16 (varlen only); it
                                         // picks rope_append_varlen_bf16_kernel / _kv8_bf16_kernel and nothing else
  bool pos = false;                      // lc_rope_append_varlen_pos_* (DESIGN.md §4.3o): the cos_sin row of token t is pos_ids[t], not its cache slot (varlen
                                         // only); it picks the rope_append_varlen_pos_*kernel and adds RopeAppendPtrs::pos_ids to the NULL check
};
struct RopeAppendPtrs {
  AppendPtrs a;
  const half_t* Q;                       // dense [B,H,Nq,D], or (packed) a token-major projection output, as a.Knew and a.Vnew
  half_t* Qout;                          // dense [B,H,Nq,D]; may be Q itself for a dense source
  const float* cos_sin;                  // device float[max_pos, rot_dim]
  const int* cu_q = nullptr;             // a varlen call: device int32[B + 1]; else nullptr
  const int* pos_ids = nullptr;          // a call with RopeAppendCall::pos: device int32[T]; else nullptr
};
// The checks of the two entry points in the order that decides the status of a doubly-bad call; everything the append call shares is
// check_kv_append's, so a pool geometry that append accepts is accepted here.  p: the run call's pointers (nullptr: a name call)
int check_rope_append(const RopeAppendCall& c, const RopeAppendPtrs* p);
void format_rope_append(const RopeAppendCall& c, char* buf, int buflen);   // "rope_append_paged_kernel<128,false>" / "rope_append_paged_kv8_kernel<64,true>"
int launch_rope_append(const RopeAppendCall& c, const RopeAppendPtrs& p);  // tu_rope_append.hip; checked arguments; a varlen call: ...
// ... tu_rope_append_varlen_impl.h, instantiated once in each unit that holds such kernels: tu_rope_append_varlen.hip (fp16), tu_rope_append_varlen_bf16.hip
// and tu_rope_append_varlen_pos.hip (RopeAppendCall::pos, fp16 and bf16)
enum class RopeVarlenUnit { F16, BF16, POS };
template <RopeVarlenUnit U>
int launch_rope_append_varlen(const RopeAppendCall& c, const RopeAppendPtrs& p);

}  // namespace lc
