// lc_abi.hip — the C-ABI of libleetcuda_amd.so (declared in include/lc_abi.h): each entry point states its call, has it checked and planned, asks the
// launch guard and launches the plan; the knob and entry-table calls; HIP-event timing helpers.  What a call runs is decided in tu_plan.hip (lc_plan.h) and
// launched by tu_core.hip and the other tu_*.hip units (lc_launch.h); this unit holds no launch decision and no kernel.
// Host side of the reference's L2 layer (the `void f(torch::Tensor...)` wrappers at the tail of every
// reference .cu, e.g. kernels/hgemm/mma/basic/hgemm_mma_stage.cu:2331-2412 and
// kernels/flash-attn/mma/basic/flash_attn_mma_split_q.cu:701-815) re-expressed on raw pointers.
#include "../../include/lc_abi.h"

#include <string.h>

#include <new>

#include "lc_plan.h"

using namespace lc;

namespace {

// one HGEMM call on one knob snapshot (lc_hgemm_f16, lc_hgemm_call)
int hgemm_f16(const Knobs& k, const void* A, const void* B, void* C, int M, int N, int K, int layout, int variant, int swizzle_stride, void* stream) {
  if (!A || !B || !C) return LC_ERR_ARG;
  if (layout != LC_LAYOUT_NN && layout != LC_LAYOUT_TN) return LC_ERR_ARG;
  if (!is_hgemm_variant(variant)) return LC_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0) return LC_ERR_SHAPE;
  const bool al = aligned16(A) && aligned16(B) && aligned16(C);
  HgemmPlan p;
  if (int rc = plan_hgemm(k, M, N, K, layout == LC_LAYOUT_NN, variant, al, &p)) return rc;
  if (int rc = launch_guard()) return rc;   // a sticky HIP error of an earlier call: report it, launch nothing
  return launch_hgemm(p, static_cast<const half_t*>(A), static_cast<const half_t*>(B), static_cast<half_t*>(C), M, N, K, layout == LC_LAYOUT_NN,
                      swizzle_stride, static_cast<hipStream_t>(stream));
}

constexpr int kAttnFlags = LC_ATTN_CAUSAL | LC_ATTN_V_TRANSPOSED;   // the flags of the _ex / _gqa calls

// The argument checks of the attention entry points; their order decides which status a doubly-bad call gets.  Hkv: the K / V heads (H: not a
// grouped-query call); grid_factor: what the 1-D grid bound multiplies the 64-row query blocks by (lc_attn_fwd_bf16: 4).
int check_attn_args(const void* Q, const void* K, const void* V, const void* O, int B, int H, int Hkv, int N, int D, int grid_factor) {
  if (!Q || !K || !V || !O) return LC_ERR_ARG;
  if (H <= 0 || Hkv < 1 || Hkv > H || H % Hkv != 0) return LC_ERR_SHAPE;
  if (B <= 0 || N <= 0 || D <= 0) return LC_ERR_SHAPE;
  if (N % KVB != 0) return LC_ERR_SHAPE;
  if ((size_t)B * H * (size_t)(N / 64) * grid_factor > 0x7fffffffull) return LC_ERR_SHAPE;  // 1-D grid of workgroups
  if (!attn_span_fits(N, D)) return LC_ERR_SHAPE;
  if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O)) return LC_ERR_SHAPE;
  if (Hkv != H && !is_small_headdim(D)) return LC_ERR_HEADDIM;   // (D >= 256: no grouped-query kernels yet)
  return LC_OK;
}

// one attention call on checked arguments (bf16: raw 16-bit lanes, the kernel flavour decodes them; c.gqa > 1: K / V hold H / c.gqa heads)
int attn_fwd(const void* Q, const void* K, const void* V, void* O, const AttnCall& c, void* stream) {
  if (int rc = launch_guard()) return rc;
  AttnPlan p;
  if (int rc = plan_attn(read_knobs(), c, &p)) return rc;
  return launch_attn_plan(p, AttnPtrs{static_cast<const half_t*>(Q), static_cast<const half_t*>(K), static_cast<const half_t*>(V), static_cast<half_t*>(O),
                                      static_cast<hipStream_t>(stream)});
}

// The name calls: the buffer, group (G = H / Hkv, 1: not a grouped-query call), N, span and head-dim checks in the order of the forward call they
// mirror; bad_n: the status of a bad N — LC_ERR_ARG for lc_attn_kernel_name[_bh], LC_ERR_SHAPE (what the forward call returns) for the newer calls.
int attn_name(int BH, int G, int N, int D, int flags, bool bf16, int bad_n, char* buf, int buflen) {
  if (!buf || buflen < 8) return LC_ERR_ARG;
  if (G < 1 || (BH > 0 && BH % G != 0)) return LC_ERR_SHAPE;
  if (N <= 0 || N % KVB != 0) return bad_n;
  if (!attn_span_fits(N, D)) return LC_ERR_SHAPE;
  if (G != 1 && !is_small_headdim(D)) return LC_ERR_HEADDIM;
  AttnPlan p;
  if (int rc = plan_attn(read_knobs(), AttnCall{BH > 0 ? (long)BH : -1, G, N, D, (flags & LC_ATTN_V_TRANSPOSED) != 0, bf16, (flags & LC_ATTN_CAUSAL) != 0}, &p))
    return rc;
  format_attn(p, buf, buflen);
  return LC_OK;
}

// The three decode families (contiguous, paged, paged fp8) each state a DecodeCall; check_attn_decode (tu_plan.hip) checks and plans it; decode_run,
// decode_bytes and decode_name run, size and name the plan.  (DecodeCall: B, H, Hkv, Nq, D, flags, kv_bytes, paged, Ncap, num_pages, page_size, max_pages)
// chunk: the lc_attn_chunk_* entries — the same call with R = (H / Hkv) x Nq unbounded
DecodeCall decode_flat(int B, int H, int Hkv, int Nq, int Ncap, int D, int flags, bool chunk = false) {
  return DecodeCall{B, H, Hkv, Nq, D, flags, 2, false, Ncap, 0, 0, 0, chunk};
}
DecodeCall decode_paged(int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D, int flags, int kv_bytes, bool chunk = false) {
  return DecodeCall{B, H, Hkv, Nq, D, flags, kv_bytes, true, 0, num_pages, page_size, max_pages, chunk};
}
// the lc_attn_local_* entries: the chunk call c with a window and, a run call, its sinks (window = 0, no sinks: c itself)
DecodeCall decode_local(DecodeCall c, int window, const float* sinks = nullptr) {
  c.window = window;
  c.sinks = sinks != nullptr;
  return c;
}
// What a ragged entry (lc_attn_varlen_paged_*, lc_rope_append_varlen_*) is a variant of, as a set of bits: its name says them
enum : unsigned {
  VL_F16 = 0,             // fp16 elements, 16-bit pools, O alone (attention) / the cache slot as rotary position (rope)
  VL_KV8 = 1,             // *_kv8: e4m3 pools under k_scale, v_scale
  VL_BF16 = 2,            // *_bf16: the same call on bfloat16 elements
  VL_LSE = 4,             // lc_attn_varlen_paged_lse_* (§4.3n): the same call, which also writes each row's log-sum-exp
  VL_TREE = 8 | VL_LSE,   // lc_attn_varlen_paged_tree_* (§4.3o): the lse call with a look-back visibility word per query token
  VL_POS = 16             // lc_rope_append_varlen_pos_* (§4.3o): the rotary position of token t is pos_ids[t]
};
// the lc_attn_varlen_paged_* entries: the paged local call of Nq = max_nq on T token-major rows.  The query calls state
// num_pages = 1 and sinks = nullptr
DecodeCall varlen_call(unsigned variant, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
                       const float* sinks, int flags) {
  DecodeCall c = decode_local(decode_paged(B, H, Hkv, max_nq, num_pages, page_size, max_pages, D, flags, variant & VL_KV8 ? 1 : 2, true), window, sinks);
  c.varlen = true;
  c.T = T;
  c.max_nq = max_nq;
  c.bf16 = (variant & VL_BF16) != 0;
  c.lse = (variant & VL_LSE) != 0;
  c.tree = (variant & VL_TREE) == VL_TREE;
  return c;
}
// block_table: paged calls; k_scale / v_scale: the fp8 call (nullptr elsewhere); sinks: a local or varlen call, or nullptr; cu_q: a varlen call
int decode_run(const DecodeCall& c, const void* Q, const void* K, const void* V, void* O, const int* kv_len, const int* block_table, const float* k_scale,
               const float* v_scale, void* workspace, size_t workspace_bytes, void* stream, const float* sinks = nullptr, const int* cu_q = nullptr,
               float* lse = nullptr, const uint64_t* tree_mask = nullptr) {
  const DecodePtrs a{static_cast<const half_t*>(Q), K, V, static_cast<half_t*>(O), kv_len, static_cast<hipStream_t>(stream), block_table, k_scale, v_scale, sinks, cu_q, lse, tree_mask};
  DecodePlan p;
  if (int rc = check_attn_decode(c, &a, &p)) return rc;
  if (workspace && (workspace_bytes < decode_workspace_bytes(p) || !aligned16(workspace))) return LC_ERR_ARG;
  if (int rc = launch_guard()) return rc;
  return launch_attn_decode(p, a, workspace);
}
size_t decode_bytes(const DecodeCall& c) {
  DecodePlan p;
  return check_attn_decode(c, nullptr, &p) == LC_OK ? decode_workspace_bytes(p) : 0;
}
int decode_name(const DecodeCall& c, char* buf, int buflen) {
  if (!buf || buflen < 8) return LC_ERR_ARG;   // (an unknown flag has the same status: which of the two is found first cannot be told)
  DecodePlan p;
  if (int rc = check_attn_decode(c, nullptr, &p)) return rc;
  format_attn_decode(p, buf, buflen);
  return LC_OK;
}

// The two state-merge entries state a MergeCall; check_attn_merge (tu_plan.hip) checks it, launch_attn_merge (tu_attn_merge.hip) runs it
int merge_run(bool bf16, const void* Oa, const float* lse_a, const void* Ob, const float* lse_b, void* Oout, float* lse_out, const int* cu_q, int B,
              int T, int H, int D, void* stream) {
  const MergeCall c{B, T, H, D, bf16};
  const MergePtrs p{static_cast<const half_t*>(Oa), lse_a, static_cast<const half_t*>(Ob), lse_b, static_cast<half_t*>(Oout), lse_out, cu_q,
                    static_cast<hipStream_t>(stream)};
  if (int rc = check_attn_merge(c, p)) return rc;
  if (int rc = launch_guard()) return rc;
  return launch_attn_merge(c, p);
}

// The two append-to-cache entries (fp16 and fp8 pools) each state an AppendCall; check_kv_append (tu_plan.hip) checks it; append_run and append_name
// run and name it.  (AppendCall: B, Hkv, Nq, D, flags, kv_bytes, num_pages, page_size, max_pages)
int append_run(const AppendCall& c, const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int* block_table, const int* kv_len,
               const float* k_scale, const float* v_scale, void* stream) {
  const AppendPtrs a{static_cast<const half_t*>(Knew), static_cast<const half_t*>(Vnew), Kpool, Vpool, block_table, kv_len, k_scale, v_scale,
                     static_cast<hipStream_t>(stream)};
  if (int rc = check_kv_append(c, &a)) return rc;
  if (int rc = launch_guard()) return rc;
  return launch_kv_append(c, a);
}
int append_name(const AppendCall& c, char* buf, int buflen) {
  if (!buf || buflen < 8) return LC_ERR_ARG;
  if (int rc = check_kv_append(c, nullptr)) return rc;
  format_kv_append(c, buf, buflen);
  return LC_OK;
}

// The two rotary-embedding + append entries each state a RopeAppendCall (an AppendCall with flags 0 + H, rot_dim, max_pos, src_row_stride, flags);
// check_rope_append (tu_plan.hip) checks it; rope_run and rope_name run and name it.
RopeAppendCall rope_call(int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                         long long src_row_stride, int flags, int kv_bytes) {
  return RopeAppendCall{AppendCall{B, Hkv, Nq, D, 0, kv_bytes, num_pages, page_size, max_pages}, H, rot_dim, max_pos, src_row_stride, flags};
}
int rope_run(const RopeAppendCall& c, const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool, const float* cos_sin,
             const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale, void* stream) {
  const RopeAppendPtrs p{AppendPtrs{static_cast<const half_t*>(Knew), static_cast<const half_t*>(Vnew), Kpool, Vpool, block_table, kv_len, k_scale, v_scale,
                                    static_cast<hipStream_t>(stream)},
                         static_cast<const half_t*>(Q), static_cast<half_t*>(Qout), cos_sin};
  if (int rc = check_rope_append(c, &p)) return rc;
  if (int rc = launch_guard()) return rc;
  return launch_rope_append(c, p);
}
// the lc_rope_append_varlen_* entries: the rope call of Nq = max_nq on T token-major rows with a stride each
RopeAppendCall rope_varlen_call(unsigned variant, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int rot_dim,
                                int max_pos, long long q_row_stride, long long kv_row_stride, int flags) {
  RopeAppendCall c = rope_call(B, H, Hkv, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, flags, variant & VL_KV8 ? 1 : 2);
  c.varlen = true;
  c.T = T;
  c.max_nq = max_nq;
  c.kv_row_stride = kv_row_stride;
  c.bf16 = (variant & VL_BF16) != 0;
  c.pos = (variant & VL_POS) != 0;
  return c;
}
int rope_varlen_run(const RopeAppendCall& c, const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool,
                    const float* cos_sin, const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale,
                    void* stream, const int* pos_ids = nullptr) {
  const RopeAppendPtrs p{AppendPtrs{static_cast<const half_t*>(Knew), static_cast<const half_t*>(Vnew), Kpool, Vpool, block_table, kv_len, k_scale, v_scale,
                                    static_cast<hipStream_t>(stream)},
                         static_cast<const half_t*>(Q), static_cast<half_t*>(Qout), cos_sin, cu_q, pos_ids};
  if (int rc = check_rope_append(c, &p)) return rc;
  if (int rc = launch_guard()) return rc;
  if (c.pos) return launch_rope_append_varlen<RopeVarlenUnit::POS>(c, p);
  return c.bf16 ? launch_rope_append_varlen<RopeVarlenUnit::BF16>(c, p) : launch_rope_append_varlen<RopeVarlenUnit::F16>(c, p);
}
int rope_name(const RopeAppendCall& c, char* buf, int buflen) {
  if (!buf || buflen < 8) return LC_ERR_ARG;
  if (int rc = check_rope_append(c, nullptr)) return rc;
  format_rope_append(c, buf, buflen);
  return LC_OK;
}

// The two fp8 GEMM entries each state a GemmFp8Call (M, N, K, swizzle_stride, mx); check_gemm_fp8 (tu_plan.hip) checks and plans it.  PA / PB: the block-scaled call
int gemm_fp8_run(const GemmFp8Call& c, const void* A, const void* PA, const void* B, const void* PB, void* C, float alpha, void* stream) {
  const GemmFp8Ptrs a{static_cast<const uint8_t*>(A), static_cast<const uint8_t*>(B), static_cast<half_t*>(C), static_cast<const uint32_t*>(PA),
                      static_cast<const uint32_t*>(PB), alpha, static_cast<hipStream_t>(stream)};
  GemmFp8Plan p;
  if (int rc = check_gemm_fp8(c, &a, &p)) return rc;
  if (int rc = launch_guard()) return rc;
  return launch_gemm_fp8_plan(p, a);
}

// warmup + iters calls of `launch` (returns a status) between two events (lc_hgemm_time, lc_attn_time): ms per timed call
template <typename Launch>
int time_launches(int warmup, int iters, void* stream, float* ms_per_launch, Launch launch) {
  if (!ms_per_launch || iters <= 0 || warmup < 0) return LC_ERR_ARG;
  for (int i = 0; i < warmup; ++i)
    if (int rc = launch()) return rc;
  void* t = nullptr;
  if (int rc = lc_timer_start(stream, &t)) return rc;
  int rc = LC_OK;
  for (int i = 0; i < iters && rc == LC_OK; ++i) rc = launch();
  float ms = 0.f;
  const int rc2 = lc_timer_stop(t, &ms);
  *ms_per_launch = ms / iters;
  return rc != LC_OK ? rc : rc2;
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// vendor comparator (hipBLASLt), resolved lazily with dlopen so the core library has no link-time
// dependency on it.

#include "vendor_gemm.inc"

extern "C" {

int lc_abi_version(void) { return LC_ABI_VERSION; }

const char* lc_status_string(int status) {
  switch (status) {
    case LC_OK: return "ok";
    case LC_ERR_ARG: return "invalid argument";
    case LC_ERR_SHAPE: return "Tensor size mismatch!";
    case LC_ERR_HEADDIM: return "headdim not support!";
    case LC_ERR_LAUNCH: return "kernel launch failed";
    case LC_ERR_VENDOR: return "vendor GEMM (hipBLASLt) unavailable or failed";
    case LC_ERR_DEVICE: return "no gfx950 device";
    default: return "unknown status";
  }
}

const char* lc_build_info(int* is_diag) {
#ifdef LC_DIAG
  if (is_diag) *is_diag = 1;
  return "gfx950 -O3 LC_DIAG=1 (diagnosis build: ablation / stamp kernels compiled in)";
#else
  if (is_diag) *is_diag = 0;
  return "gfx950 -O3 LC_DIAG=0";
#endif
}

int lc_hgemm_kernel_name(int M, int N, int K, int layout, int variant, char* buf, int buflen) {
  if (!buf || buflen < 8 || M <= 0 || N <= 0 || K <= 0 || !is_hgemm_variant(variant)) return LC_ERR_ARG;
  if (layout != LC_LAYOUT_NN && layout != LC_LAYOUT_TN) return LC_ERR_ARG;
  HgemmPlan p;
  if (int rc = plan_hgemm(read_knobs(), M, N, K, layout == LC_LAYOUT_NN, variant, true, &p)) return rc;
  format_hgemm(p, M, N, layout == LC_LAYOUT_NN, buf, buflen);
  return LC_OK;
}

int lc_attn_kernel_name(int N, int D, int v_transposed, int bf16, char* buf, int buflen) {
  return lc_attn_kernel_name_bh(-1, N, D, v_transposed, bf16, buf, buflen);
}

int lc_attn_kernel_name_bh(int BH, int N, int D, int v_transposed, int bf16, char* buf, int buflen) {
  return attn_name(BH, 1, N, D, v_transposed ? LC_ATTN_V_TRANSPOSED : 0, bf16 != 0, LC_ERR_ARG, buf, buflen);
}

int lc_attn_kernel_name_ex(int BH, int N, int D, int flags, char* buf, int buflen) {
  return lc_attn_kernel_name_gqa(BH, 1, N, D, flags, buf, buflen);
}

int lc_attn_kernel_name_gqa(int BH, int G, int N, int D, int flags, char* buf, int buflen) {
  if (flags & ~kAttnFlags) return LC_ERR_ARG;
  // (G = 1 without the causal flag IS lc_attn_kernel_name_bh, its status for a bad N included)
  return attn_name(BH, G, N, D, flags, false, G == 1 && !(flags & LC_ATTN_CAUSAL) ? LC_ERR_ARG : LC_ERR_SHAPE, buf, buflen);
}

int lc_tune_set(const char* key, int value) {
  const Knob* k = find_knob(key);
  if (!k || !k->valid(value)) return LC_ERR_ARG;
  k->var->store(value, std::memory_order_relaxed);
  return LC_OK;
}

int lc_tune_get(const char* key, int* value, int* default_value) {
  const Knob* k = find_knob(key);
  if (!k) return LC_ERR_ARG;
  if (value) *value = k->var->load(std::memory_order_relaxed);
  if (default_value) *default_value = k->dflt;
  return LC_OK;
}

int lc_tune_count(void) { return kNumKnobs; }
size_t lc_workspace_release(void) { return workspace_release_all(); }
size_t lc_workspace_bytes(void) { return workspace_cached_bytes(); }
const char* lc_tune_key(int index) {
  if (index < 0 || index >= lc_tune_count()) return nullptr;
#ifndef LC_DIAG
  if (kKnobs[index].diag) return nullptr;
#endif
  return kKnobs[index].key;
}

int lc_device_check(int* num_cus) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return LC_ERR_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return LC_ERR_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return LC_ERR_DEVICE;
  if (num_cus) *num_cus = prop.multiProcessorCount;
  return LC_OK;
}

int lc_hgemm_f16(const void* A, const void* B, void* C, int M, int N, int K, int layout, int variant,
                 int stages, int swizzle_stride, void* stream) {
  (void)stages;  // accepted and ignored: the LDS ring depth is fixed per kernel family (lc_abi.h)
  return hgemm_f16(read_knobs(), A, B, C, M, N, K, layout, variant, swizzle_stride, stream);
}

int lc_gemm_fp8_e4m3(const void* A, const void* B, void* C, int M, int N, int K, float alpha, int swizzle_stride, void* stream) {
  return gemm_fp8_run(GemmFp8Call{M, N, K, swizzle_stride, false}, A, nullptr, B, nullptr, C, alpha, stream);
}

int lc_mxfp8_pack_scales(const void* S, void* P, int rows, int K, void* stream) {
  if (int rc = check_mx_pack_scales(S, P, rows, K)) return rc;
  if (int rc = launch_guard()) return rc;
  return launch_mx_pack_scales(static_cast<const uint8_t*>(S), static_cast<uint32_t*>(P), rows, K, static_cast<hipStream_t>(stream));
}

int lc_gemm_mxfp8(const void* A, const void* PA, const void* B, const void* PB, void* C, int M, int N, int K, float alpha, int swizzle_stride, void* stream) {
  return gemm_fp8_run(GemmFp8Call{M, N, K, swizzle_stride, true}, A, PA, B, PB, C, alpha, stream);
}

int lc_hgemm_entry_count(void) { return kNumHgemmEntries; }
const char* lc_hgemm_entry_name(int index) {
  return (index >= 0 && index < kNumHgemmEntries) ? kHgemmEntries[index].name : nullptr;
}
int lc_hgemm_entry_info(const char* entry, int* layout, int* nargs) {
  const HgemmEntry* e = find_hgemm(entry);
  if (!e) return LC_ERR_ARG;
  if (layout) *layout = e->layout;
  if (nargs) *nargs = e->nargs;
  return LC_OK;
}

int lc_hgemm_call(const char* entry, const void* A, const void* B, void* C, int M, int N, int K,
                  int stages, int swizzle, int swizzle_stride, void* stream) {
  (void)stages;  // (ignored, as by lc_hgemm_f16)
  const HgemmEntry* e = find_hgemm(entry);
  if (!e) return LC_ERR_ARG;
  if (e->variant == -2) return lc_vendor_init();
  if (e->variant == -3) return lc_vendor_destroy();
  if (e->variant == -1) return lc_hgemm_vendor_f16(A, B, C, M, N, K, e->layout, stream);
  const Knobs k = read_knobs();
  const int variant = hgemm_entry_variant(k, *e, M, N, K, aligned16(A) && aligned16(B) && aligned16(C));   // (the name's own, or what serves the shape)
  const int stride = (e->nargs == 6 && swizzle) ? swizzle_stride : 1;
  return hgemm_f16(k, A, B, C, M, N, K, e->layout, variant, stride, stream);
}

int lc_attn_fwd_f16(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                    int v_transposed, int family, int acc_f32, int stages, void* stream) {
  (void)acc_f32;
  (void)stages;
  // (the family range check sits between the null check and the shape checks: both of its neighbours' LC_ERR_ARG outrank LC_ERR_SHAPE)
  const int rc = check_attn_args(Q, K, V, O, B, H, H, N, D, 1);
  if (rc == LC_ERR_ARG || family < LC_ATTN_SPLIT_Q || family > LC_ATTN_SPLIT_KV) return LC_ERR_ARG;
  if (rc) return rc;
  return attn_fwd(Q, K, V, O, AttnCall{(long)B * H, 1, N, D, v_transposed != 0, false, false}, stream);
}

int lc_attn_fwd_f16_ex(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int flags, void* stream) {
  return lc_attn_fwd_f16_gqa(Q, K, V, O, B, H, H, N, D, flags, stream);
}

// Hkv = H IS the MHA call: same checks, plan, kernel and bits
int lc_attn_fwd_f16_gqa(const void* Q, const void* K, const void* V, void* O, int B, int H, int Hkv, int N, int D, int flags, void* stream) {
  if (flags & ~kAttnFlags) return LC_ERR_ARG;
  if (int rc = check_attn_args(Q, K, V, O, B, H, Hkv, N, D, 1)) return rc;
  return attn_fwd(Q, K, V, O, AttnCall{(long)B * H, H / Hkv, N, D, (flags & LC_ATTN_V_TRANSPOSED) != 0, false, (flags & LC_ATTN_CAUSAL) != 0}, stream);
}

int lc_attn_decode_f16(const void* Q, const void* K, const void* V, void* O, const int* kv_len, int B, int H, int Hkv, int Nq, int Ncap, int D,
                       int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_flat(B, H, Hkv, Nq, Ncap, D, flags), Q, K, V, O, kv_len, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

size_t lc_attn_decode_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int D) { return decode_bytes(decode_flat(B, H, Hkv, Nq, Ncap, D, 0)); }

int lc_attn_decode_kernel_name(int B, int H, int Hkv, int Nq, int Ncap, int D, int flags, char* buf, int buflen) {
  return decode_name(decode_flat(B, H, Hkv, Nq, Ncap, D, flags), buf, buflen);
}

int lc_attn_decode_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, const int* block_table, const int* kv_len, int B, int H,
                             int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D, int flags, void* workspace, size_t workspace_bytes,
                             void* stream) {
  return decode_run(decode_paged(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, flags, 2), Q, Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr,
                    workspace, workspace_bytes, stream);
}

// (the two query calls of a paged family take no num_pages: it decides nothing)
size_t lc_attn_decode_paged_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D) {
  return decode_bytes(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, 0, 2));
}

int lc_attn_decode_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int flags, char* buf, int buflen) {
  return decode_name(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, flags, 2), buf, buflen);
}

int lc_attn_decode_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, const int* block_table, const int* kv_len,
                             const float* k_scale, const float* v_scale, int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages,
                             int D, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_paged(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, flags, 1), Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale,
                    workspace, workspace_bytes, stream);
}

size_t lc_attn_decode_paged_kv8_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D) {
  return decode_bytes(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, 0, 1));
}

int lc_attn_decode_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int flags, char* buf, int buflen) {
  return decode_name(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, flags, 1), buf, buflen);
}

// The chunk entries: the decode entries' DecodeCall with chunk = true (R <= 64: the decode call's plan, name and bits)
int lc_attn_chunk_f16(const void* Q, const void* K, const void* V, void* O, const int* kv_len, int B, int H, int Hkv, int Nq, int Ncap, int D,
                      int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_flat(B, H, Hkv, Nq, Ncap, D, flags, true), Q, K, V, O, kv_len, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

size_t lc_attn_chunk_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int D) { return decode_bytes(decode_flat(B, H, Hkv, Nq, Ncap, D, 0, true)); }

int lc_attn_chunk_kernel_name(int B, int H, int Hkv, int Nq, int Ncap, int D, int flags, char* buf, int buflen) {
  return decode_name(decode_flat(B, H, Hkv, Nq, Ncap, D, flags, true), buf, buflen);
}

int lc_attn_chunk_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, const int* block_table, const int* kv_len, int B, int H,
                            int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D, int flags, void* workspace, size_t workspace_bytes,
                            void* stream) {
  return decode_run(decode_paged(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, flags, 2, true), Q, Kpool, Vpool, O, kv_len, block_table, nullptr,
                    nullptr, workspace, workspace_bytes, stream);
}

size_t lc_attn_chunk_paged_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D) {
  return decode_bytes(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, 0, 2, true));
}

int lc_attn_chunk_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int flags, char* buf, int buflen) {
  return decode_name(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, flags, 2, true), buf, buflen);
}

int lc_attn_chunk_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, const int* block_table, const int* kv_len,
                            const float* k_scale, const float* v_scale, int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages,
                            int D, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_paged(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, flags, 1, true), Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale,
                    v_scale, workspace, workspace_bytes, stream);
}

size_t lc_attn_chunk_paged_kv8_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D) {
  return decode_bytes(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, 0, 1, true));
}

int lc_attn_chunk_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int flags, char* buf, int buflen) {
  return decode_name(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, flags, 1, true), buf, buflen);
}

// The local entries: the chunk entries' DecodeCall with a window and sinks (neither: the chunk call's plan, name and bits)
int lc_attn_local_f16(const void* Q, const void* K, const void* V, void* O, const int* kv_len, int B, int H, int Hkv, int Nq, int Ncap, int D,
                      int window, const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_local(decode_flat(B, H, Hkv, Nq, Ncap, D, flags, true), window, sinks), Q, K, V, O, kv_len, nullptr, nullptr, nullptr, workspace,
                    workspace_bytes, stream, sinks);
}

size_t lc_attn_local_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int D, int window) {
  return decode_bytes(decode_local(decode_flat(B, H, Hkv, Nq, Ncap, D, window > 0 ? LC_ATTN_CAUSAL : 0, true), window));
}

int lc_attn_local_kernel_name(int B, int H, int Hkv, int Nq, int Ncap, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(decode_local(decode_flat(B, H, Hkv, Nq, Ncap, D, flags, true), window), buf, buflen);
}

int lc_attn_local_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, const int* block_table, const int* kv_len, int B, int H,
                            int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_local(decode_paged(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, flags, 2, true), window, sinks), Q, Kpool, Vpool, O, kv_len,
                    block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks);
}

size_t lc_attn_local_paged_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window) {
  return decode_bytes(decode_local(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, window > 0 ? LC_ATTN_CAUSAL : 0, 2, true), window));
}

int lc_attn_local_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(decode_local(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, flags, 2, true), window), buf, buflen);
}

int lc_attn_local_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, const int* block_table, const int* kv_len,
                            const float* k_scale, const float* v_scale, int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages,
                            int D, int window, const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(decode_local(decode_paged(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, flags, 1, true), window, sinks), Q, Kpool8, Vpool8, O,
                    kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks);
}

size_t lc_attn_local_paged_kv8_workspace_bytes(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window) {
  return decode_bytes(decode_local(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, window > 0 ? LC_ATTN_CAUSAL : 0, 1, true), window));
}

int lc_attn_local_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int window, int flags, char* buf,
                                        int buflen) {
  return decode_name(decode_local(decode_paged(B, H, Hkv, Nq, 1, page_size, max_pages, D, flags, 1, true), window), buf, buflen);
}

// The varlen entries: the paged local entries' DecodeCall of Nq = max_nq, with cu_q and T (no contiguous form: a ragged batch lives on a paged cache)
int lc_attn_varlen_paged_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, const int* cu_q, const int* block_table, const int* kv_len,
                             int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
                             const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_F16, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags), Q,
                    Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks, cu_q);
}

size_t lc_attn_varlen_paged_workspace_bytes(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window) {
  return decode_bytes(varlen_call(VL_F16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, window > 0 ? LC_ATTN_CAUSAL : 0));
}

int lc_attn_varlen_paged_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf,
                                     int buflen) {
  return decode_name(varlen_call(VL_F16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, const int* cu_q, const int* block_table,
                             const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages,
                             int page_size, int max_pages, int D, int window, const float* sinks, int flags, void* workspace, size_t workspace_bytes,
                             void* stream) {
  return decode_run(varlen_call(VL_KV8, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags), Q,
                    Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks, cu_q);
}

size_t lc_attn_varlen_paged_kv8_workspace_bytes(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window) {
  return decode_bytes(varlen_call(VL_KV8, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, window > 0 ? LC_ATTN_CAUSAL : 0));
}

int lc_attn_varlen_paged_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf,
                                         int buflen) {
  return decode_name(varlen_call(VL_KV8, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

// The bfloat16 varlen entries: the two entries above, argument for argument, as a DecodeCall with bf16 = true.  The checks,
// the plan and the workspace bytes are the fp16 call's (lc_attn_varlen_paged_workspace_bytes / _kv8_workspace_bytes serve both)
int lc_attn_varlen_paged_bf16(const void* Q, const void* Kpool, const void* Vpool, void* O, const int* cu_q, const int* block_table, const int* kv_len,
                              int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
                              const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_BF16, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks, cu_q);
}

int lc_attn_varlen_paged_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags,
                                          char* buf, int buflen) {
  return decode_name(varlen_call(VL_BF16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_kv8_bf16(const void* Q, const void* Kpool8, const void* Vpool8, void* O, const int* cu_q, const int* block_table,
                                  const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int T, int max_nq,
                                  int num_pages, int page_size, int max_pages, int D, int window, const float* sinks, int flags, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_KV8 | VL_BF16, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks, cu_q);
}

int lc_attn_varlen_paged_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags,
                                              char* buf, int buflen) {
  return decode_name(varlen_call(VL_KV8 | VL_BF16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

// The varlen entries that also write each row's log-sum-exp: the four entries above with `lse` right behind O, as a DecodeCall
// with lse = true.  The checks (lse joins the NULL check), the plan and the workspace bytes are the twin's; the kernels and their names are the
// twin's with "_lse" in them
int lc_attn_varlen_paged_lse_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const int* cu_q, const int* block_table,
    const int* kv_len, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
    const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_LSE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks, cu_q, lse);
}

int lc_attn_varlen_paged_lse_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_LSE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_lse_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse, const int* cu_q, const int* block_table,
    const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
    const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_KV8 | VL_LSE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks, cu_q, lse);
}

int lc_attn_varlen_paged_lse_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_KV8 | VL_LSE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_lse_bf16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const int* cu_q, const int* block_table,
    const int* kv_len, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
    const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_BF16 | VL_LSE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks, cu_q, lse);
}

int lc_attn_varlen_paged_lse_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_BF16 | VL_LSE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_lse_kv8_bf16(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse, const int* cu_q, const int* block_table,
    const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
    const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_KV8 | VL_BF16 | VL_LSE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks, cu_q, lse);
}

int lc_attn_varlen_paged_lse_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_KV8 | VL_BF16 | VL_LSE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

// The varlen entries with a look-back visibility mask per query token: the four lse entries above with `tree_mask` right behind
// lse, as a DecodeCall with lse = true and tree = true.  tree_mask joins the NULL and alignment checks and LC_ATTN_CAUSAL is required; the plan
// and the workspace bytes are the twin's; the kernels and their names are the twin's with "tree" in place of "lse"
int lc_attn_varlen_paged_tree_f16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const uint64_t* tree_mask, const int* cu_q,
    const int* block_table, const int* kv_len, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
    const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_TREE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks, cu_q, lse, tree_mask);
}

int lc_attn_varlen_paged_tree_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_TREE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_tree_kv8(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse, const uint64_t* tree_mask, const int* cu_q,
    const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size,
    int max_pages, int D, int window, const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_KV8 | VL_TREE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks, cu_q, lse, tree_mask);
}

int lc_attn_varlen_paged_tree_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_KV8 | VL_TREE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_tree_bf16(const void* Q, const void* Kpool, const void* Vpool, void* O, float* lse, const uint64_t* tree_mask, const int* cu_q,
    const int* block_table, const int* kv_len, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int window,
    const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_BF16 | VL_TREE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool, Vpool, O, kv_len, block_table, nullptr, nullptr, workspace, workspace_bytes, stream, sinks, cu_q, lse, tree_mask);
}

int lc_attn_varlen_paged_tree_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_BF16 | VL_TREE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

int lc_attn_varlen_paged_tree_kv8_bf16(const void* Q, const void* Kpool8, const void* Vpool8, void* O, float* lse, const uint64_t* tree_mask, const int* cu_q,
    const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size,
    int max_pages, int D, int window, const float* sinks, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_run(varlen_call(VL_KV8 | VL_BF16 | VL_TREE, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, window, sinks, flags),
                    Q, Kpool8, Vpool8, O, kv_len, block_table, k_scale, v_scale, workspace, workspace_bytes, stream, sinks, cu_q, lse, tree_mask);
}

int lc_attn_varlen_paged_tree_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int window, int flags, char* buf, int buflen) {
  return decode_name(varlen_call(VL_KV8 | VL_BF16 | VL_TREE, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, window, nullptr, flags), buf, buflen);
}

// The merge of two (O, lse) states over disjoint key sets (attn_merge.hip): merge_run above states a MergeCall
int lc_attn_merge_states_f16(const void* Oa, const float* lse_a, const void* Ob, const float* lse_b, void* Oout, float* lse_out, const int* cu_q, int B,
                             int T, int H, int D, void* stream) {
  return merge_run(false, Oa, lse_a, Ob, lse_b, Oout, lse_out, cu_q, B, T, H, D, stream);
}

int lc_attn_merge_states_bf16(const void* Oa, const float* lse_a, const void* Ob, const float* lse_b, void* Oout, float* lse_out, const int* cu_q, int B,
                              int T, int H, int D, void* stream) {
  return merge_run(true, Oa, lse_a, Ob, lse_b, Oout, lse_out, cu_q, B, T, H, D, stream);
}

int lc_kv_append_paged_f16(const void* Knew, const void* Vnew, void* Kpool, void* Vpool, const int* block_table, const int* kv_len, int B, int Hkv,
                           int Nq, int num_pages, int page_size, int max_pages, int D, int flags, void* stream) {
  return append_run(AppendCall{B, Hkv, Nq, D, flags, 2, num_pages, page_size, max_pages}, Knew, Vnew, Kpool, Vpool, block_table, kv_len, nullptr, nullptr,
                    stream);
}

int lc_kv_append_paged_kv8(const void* Knew, const void* Vnew, void* Kpool8, void* Vpool8, const int* block_table, const int* kv_len,
                           const float* k_scale, const float* v_scale, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D,
                           int flags, void* stream) {
  return append_run(AppendCall{B, Hkv, Nq, D, flags, 1, num_pages, page_size, max_pages}, Knew, Vnew, Kpool8, Vpool8, block_table, kv_len, k_scale,
                    v_scale, stream);
}

// (the name calls take no num_pages: it decides nothing)
int lc_kv_append_paged_kernel_name(int B, int Hkv, int Nq, int page_size, int max_pages, int D, int flags, char* buf, int buflen) {
  return append_name(AppendCall{B, Hkv, Nq, D, flags, 2, 1, page_size, max_pages}, buf, buflen);
}

int lc_kv_append_paged_kv8_kernel_name(int B, int Hkv, int Nq, int page_size, int max_pages, int D, int flags, char* buf, int buflen) {
  return append_name(AppendCall{B, Hkv, Nq, D, flags, 1, 1, page_size, max_pages}, buf, buflen);
}

int lc_rope_append_paged_f16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool, const float* cos_sin,
                             const int* block_table, const int* kv_len, int B, int H, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int D,
                             int rot_dim, int max_pos, long long src_row_stride, int flags, void* stream) {
  return rope_run(rope_call(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, src_row_stride, flags, 2), Q, Knew, Vnew, Qout, Kpool,
                  Vpool, cos_sin, block_table, kv_len, nullptr, nullptr, stream);
}

int lc_rope_append_paged_kv8(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8, const float* cos_sin,
                             const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale, int B, int H, int Hkv, int Nq,
                             int num_pages, int page_size, int max_pages, int D, int rot_dim, int max_pos, long long src_row_stride, int flags,
                             void* stream) {
  return rope_run(rope_call(B, H, Hkv, Nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, src_row_stride, flags, 1), Q, Knew, Vnew, Qout, Kpool8,
                  Vpool8, cos_sin, block_table, kv_len, k_scale, v_scale, stream);
}

// (the name calls take no num_pages: it decides nothing)
int lc_rope_append_paged_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                     long long src_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_call(B, H, Hkv, Nq, 1, page_size, max_pages, D, rot_dim, max_pos, src_row_stride, flags, 2), buf, buflen);
}

int lc_rope_append_paged_kv8_kernel_name(int B, int H, int Hkv, int Nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                         long long src_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_call(B, H, Hkv, Nq, 1, page_size, max_pages, D, rot_dim, max_pos, src_row_stride, flags, 1), buf, buflen);
}

int lc_rope_append_varlen_f16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool, const float* cos_sin,
                              const int* cu_q, const int* block_table, const int* kv_len, int B, int H, int Hkv, int T, int max_nq, int num_pages,
                              int page_size, int max_pages, int D, int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags,
                              void* stream) {
  return rope_varlen_run(rope_varlen_call(VL_F16, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags),
                         Q, Knew, Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr, stream);
}

int lc_rope_append_varlen_kv8(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8, const float* cos_sin,
                              const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale, int B, int H,
                              int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                              long long q_row_stride, long long kv_row_stride, int flags, void* stream) {
  return rope_varlen_run(rope_varlen_call(VL_KV8, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags),
                         Q, Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale, stream);
}

// (the name calls take no num_pages: it decides nothing)
int lc_rope_append_varlen_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                      long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_F16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

int lc_rope_append_varlen_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                          long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_KV8, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

// the bfloat16 twins: the same RopeAppendCall with bf16 = true
int lc_rope_append_varlen_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool, const float* cos_sin,
                               const int* cu_q, const int* block_table, const int* kv_len, int B, int H, int Hkv, int T, int max_nq, int num_pages,
                               int page_size, int max_pages, int D, int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride,
                               int flags, void* stream) {
  return rope_varlen_run(
      rope_varlen_call(VL_BF16, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), Q, Knew,
      Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr, stream);
}

int lc_rope_append_varlen_kv8_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8, const float* cos_sin,
                                   const int* cu_q, const int* block_table, const int* kv_len, const float* k_scale, const float* v_scale, int B,
                                   int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                   long long q_row_stride, long long kv_row_stride, int flags, void* stream) {
  return rope_varlen_run(
      rope_varlen_call(VL_KV8 | VL_BF16, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), Q, Knew,
      Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale, stream);
}

int lc_rope_append_varlen_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                           long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_BF16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

int lc_rope_append_varlen_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                               long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_KV8 | VL_BF16, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

// the twins with per-token rotary positions: the same RopeAppendCall with pos = true and `pos_ids` right behind cu_q
int lc_rope_append_varlen_pos_f16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool, const float* cos_sin,
                                  const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len, int B, int H, int Hkv, int T, int max_nq,
                                  int num_pages, int page_size, int max_pages, int D, int rot_dim, int max_pos, long long q_row_stride,
                                  long long kv_row_stride, int flags, void* stream) {
  return rope_varlen_run(
      rope_varlen_call(VL_POS, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), Q,
      Knew, Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr, stream, pos_ids);
}

int lc_rope_append_varlen_pos_kv8(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8, const float* cos_sin,
                                  const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len, const float* k_scale,
                                  const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages, int D,
                                  int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream) {
  return rope_varlen_run(
      rope_varlen_call(VL_KV8 | VL_POS, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), Q,
      Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale, stream, pos_ids);
}

int lc_rope_append_varlen_pos_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool, void* Vpool, const float* cos_sin,
                                   const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len, int B, int H, int Hkv, int T,
                                   int max_nq, int num_pages, int page_size, int max_pages, int D, int rot_dim, int max_pos, long long q_row_stride,
                                   long long kv_row_stride, int flags, void* stream) {
  return rope_varlen_run(
      rope_varlen_call(VL_BF16 | VL_POS, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), Q,
      Knew, Vnew, Qout, Kpool, Vpool, cos_sin, cu_q, block_table, kv_len, nullptr, nullptr, stream, pos_ids);
}

int lc_rope_append_varlen_pos_kv8_bf16(const void* Q, const void* Knew, const void* Vnew, void* Qout, void* Kpool8, void* Vpool8, const float* cos_sin,
                                       const int* cu_q, const int* pos_ids, const int* block_table, const int* kv_len, const float* k_scale,
                                       const float* v_scale, int B, int H, int Hkv, int T, int max_nq, int num_pages, int page_size, int max_pages,
                                       int D, int rot_dim, int max_pos, long long q_row_stride, long long kv_row_stride, int flags, void* stream) {
  return rope_varlen_run(
      rope_varlen_call(VL_KV8 | VL_BF16 | VL_POS, B, H, Hkv, T, max_nq, num_pages, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), Q,
      Knew, Vnew, Qout, Kpool8, Vpool8, cos_sin, cu_q, block_table, kv_len, k_scale, v_scale, stream, pos_ids);
}

// (the name calls take no num_pages: it decides nothing)
int lc_rope_append_varlen_pos_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                          long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_POS, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

int lc_rope_append_varlen_pos_kv8_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                              long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_KV8 | VL_POS, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

int lc_rope_append_varlen_pos_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim, int max_pos,
                                               long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_BF16 | VL_POS, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

int lc_rope_append_varlen_pos_kv8_bf16_kernel_name(int B, int H, int Hkv, int T, int max_nq, int page_size, int max_pages, int D, int rot_dim,
                                                   int max_pos, long long q_row_stride, long long kv_row_stride, int flags, char* buf, int buflen) {
  return rope_name(rope_varlen_call(VL_KV8 | VL_BF16 | VL_POS, B, H, Hkv, T, max_nq, 1, page_size, max_pages, D, rot_dim, max_pos, q_row_stride, kv_row_stride, flags), buf, buflen);
}

int lc_attn_fwd_bf16(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                     void* stream) {
  if (int rc = check_attn_args(Q, K, V, O, B, H, H, N, D, 4)) return rc;
  return attn_fwd(Q, K, V, O, AttnCall{(long)B * H, 1, N, D, false, true, false}, stream);
}

int lc_attn_entry_count(void) { return kNumAttnEntries; }
const char* lc_attn_entry_name(int index) {
  return (index >= 0 && index < kNumAttnEntries) ? kAttnEntries[index].name : nullptr;
}
int lc_attn_entry_info(const char* entry, int* family, int* v_transposed, int* acc_f32,
                       int* max_d_stage2, int* max_d_stage1, int* nargs) {
  const AttnEntry* e = find_attn(entry);
  if (!e) return LC_ERR_ARG;
  if (family) *family = e->family;
  if (v_transposed) *v_transposed = e->vt;
  if (acc_f32) *acc_f32 = e->acc_f32;
  if (max_d_stage2) *max_d_stage2 = e->maxd_s2;
  if (max_d_stage1) *max_d_stage1 = e->maxd_s1;
  if (nargs) *nargs = e->nargs;
  return LC_OK;
}

int lc_attn_call(const char* entry, const void* Q, const void* K, const void* V, void* O, int B, int H,
                 int N, int D, int stages, void* stream) {
  const AttnEntry* e = find_attn(entry);
  if (!e) return LC_ERR_ARG;
  const int st2 = (e->nargs == 4) ? 2 : stages;
  const int maxd = st2 > 1 ? e->maxd_s2 : e->maxd_s1;
  if (D > maxd) return LC_ERR_HEADDIM;  // the reference wrapper's `default:` branch
  return lc_attn_fwd_f16(Q, K, V, O, B, H, N, D, e->vt, e->family, e->acc_f32, st2, stream);
}

// ------------------------------------------------------------------------------------------------
// measurement helpers: every HIP return code is checked (a faulting kernel must not turn into a plausible ms value)
struct LcTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t st = nullptr;
};

int lc_timer_start(void* stream, void** timer) {
  if (!timer) return LC_ERR_ARG;
  *timer = nullptr;
  LcTimer* t = new (std::nothrow) LcTimer();
  if (!t) return LC_ERR_LAUNCH;
  t->st = static_cast<hipStream_t>(stream);
  if (hipEventCreate(&t->e0) != hipSuccess) { delete t; return LC_ERR_LAUNCH; }
  if (hipEventCreate(&t->e1) != hipSuccess) { (void)hipEventDestroy(t->e0); delete t; return LC_ERR_LAUNCH; }
  if (hipEventRecord(t->e0, t->st) != hipSuccess) {
    (void)hipEventDestroy(t->e0); (void)hipEventDestroy(t->e1); delete t;
    return LC_ERR_LAUNCH;
  }
  *timer = t;
  return LC_OK;
}

int lc_timer_stop(void* timer, float* elapsed_ms) {
  LcTimer* t = static_cast<LcTimer*>(timer);
  if (!t) return LC_ERR_ARG;
  int rc = LC_OK;
  float ms = 0.f;
  if (hipEventRecord(t->e1, t->st) != hipSuccess) rc = LC_ERR_LAUNCH;
  if (rc == LC_OK && hipEventSynchronize(t->e1) != hipSuccess) rc = LC_ERR_LAUNCH;   // execution faults surface here
  if (rc == LC_OK && hipEventElapsedTime(&ms, t->e0, t->e1) != hipSuccess) rc = LC_ERR_LAUNCH;
  (void)hipEventDestroy(t->e0);
  (void)hipEventDestroy(t->e1);
  delete t;
  if (elapsed_ms) *elapsed_ms = ms;
  return (rc == LC_OK && !elapsed_ms) ? LC_ERR_ARG : rc;
}

int lc_hgemm_time(const void* A, const void* B, void* C, int M, int N, int K, int layout, int variant,
                  int stages, int swizzle_stride, int warmup, int iters, void* stream,
                  float* ms_per_launch) {
  return time_launches(warmup, iters, stream, ms_per_launch,
                       [&] { return lc_hgemm_f16(A, B, C, M, N, K, layout, variant, stages, swizzle_stride, stream); });
}

int lc_attn_time(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D,
                 int v_transposed, int family, int stages, int warmup, int iters, void* stream,
                 float* ms_per_launch) {
  return time_launches(warmup, iters, stream, ms_per_launch,
                       [&] { return lc_attn_fwd_f16(Q, K, V, O, B, H, N, D, v_transposed, family, 0, stages, stream); });
}

// One-time calibration of the split-KV cost model on the CURRENT device (round 6): times, on zero-filled scratch tensors, the merged-phase
// kernel on two one-round grids that differ only in the number of KV tiles (tau_D = the difference per tile, D = 128 and 64) and two split
// launches of one shape (S = 2: one round of T / 2 tiles; S = 4: two rounds of T / 4) whose excess over the walk gives the fixed cost of the
// combine and the rate at which partials are written and read back.  About 60 launches of 20 ... 60 us + 70 MiB of scratch, freed before
// returning.  Values outside [0.4, 2.5] x the built-in constants are REFUSED (a busy or throttled GPU): the built-in constants then stay.
// out4 (optional): tau128, tau64, x0 (us), bytes per us — of what the rule will use from now on.  Returns LC_OK when the measured values
// were adopted, LC_ERR_DEVICE without a gfx950 device, LC_ERR_LAUNCH on a HIP error, LC_ERR_ARG when they were refused.
int lc_tune_calibrate(void* stream, float* out4) {
  int ncu = 0;
  if (int rc = lc_device_check(&ncu)) return rc;
  if (int rc = launch_guard()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stream_is_capturing(st)) return LC_ERR_ARG;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LC_ERR_DEVICE;
  const int bh1 = ncu / 4 > 0 ? ncu / 4 : 1;                       // N = 1024: 4 blocks per head -> one round
  const size_t elems = (size_t)bh1 * 1024 * 128;                    // the largest tensor any step uses
  half_t* buf = nullptr;
  {
    RelaxedCaptureMode relaxed;
    if (hipMalloc(&buf, 4 * elems * sizeof(half_t)) != hipSuccess || !buf) {
      (void)hipGetLastError();
      return LC_ERR_LAUNCH;
    }
  }
  int rc = LC_OK;
  if (hipMemsetAsync(buf, 0, 4 * elems * sizeof(half_t), st) != hipSuccess) rc = LC_ERR_LAUNCH;
  half_t *q = buf, *k = buf + elems, *v = buf + 2 * elems, *o = buf + 3 * elems;
  const AttnPtrs ptrs{q, k, v, o, st};
  auto time_us = [&](int D, int bh, int N, int walk, int ns, double* us) -> int {
    const AttnW4uUnit* unit = find_attn_w4u(D, false, false);   // (D = 128 / 64)
    auto once = [&]() -> int { return unit->launch(ptrs, bh, N, walk, ns, 1); };
    for (int i = 0; i < 3; ++i)
      if (int r = once()) return r;
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {   // best of three bursts of four: a burst shares its launch gaps, the minimum sheds a preempted one
      void* t = nullptr;
      if (int r = lc_timer_start(st, &t)) return r;
      int r2 = LC_OK;
      for (int i = 0; i < 4 && r2 == LC_OK; ++i) r2 = once();
      float ms = 0.f;
      const int r3 = lc_timer_stop(t, &ms);
      if (r2 != LC_OK) return r2;
      if (r3 != LC_OK) return r3;
      if (ms * 250.0 < best) best = ms * 250.0;   // us per launch
    }
    *us = best;
    return LC_OK;
  };
  double tau[2] = {0, 0}, x0 = 0, bpu = 0;
  for (int di = 0; di < 2 && rc == LC_OK; ++di) {
    const int D = di == 0 ? 128 : 64;
    double t16 = 0, t32 = 0;
    rc = time_us(D, bh1, 1024, 0, 1, &t16);                                  // ncu blocks x 16 tiles
    if (rc == LC_OK) rc = time_us(D, bh1 / 2 > 0 ? bh1 / 2 : 1, 2048, 0, 1, &t32);   // ncu blocks x 32 tiles
    tau[di] = (t32 - t16) / 16.0;
  }
  if (rc == LC_OK) {
    // (1, ncu / 16, 2048, 128): g = ncu / 2 blocks of T = 32 tiles; S = 2 -> one round of 16 tiles, S = 4 -> two rounds of 8
    const int bh = ncu / 16 > 0 ? ncu / 16 : 1;
    const double part = 4.0 * bh * 2048 * 128;
    double t2 = 0, t4 = 0;
    rc = time_us(128, bh, 2048, 3, 2, &t2);
    if (rc == LC_OK) rc = time_us(128, bh, 2048, 3, 4, &t4);
    const double e2 = t2 - 16.0 * tau[0], e4 = t4 - 2 * 8.0 * tau[0];       // = x0 + S part / bw
    const double per = (e4 - e2) / 2.0;                                       // part / bw
    bpu = per > 0 ? part / per : 0;
    x0 = e2 - 2.0 * per;
  }
  (void)hipStreamSynchronize(st);
  {
    RelaxedCaptureMode relaxed;
    (void)hipFree(buf);
  }
  if (rc != LC_OK) return rc;
  auto sane = [](double v, double ref) { return v >= 0.4 * ref && v <= 2.5 * ref; };
  const bool ok = sane(tau[0], 1.35) && sane(tau[1], 0.85) && sane(x0, kSplitFixedUs) && sane(bpu, kSplitBytesPerUs);
  AttnCalib& c = g_attn_calib[dev];
  if (ok) {
    c.valid.store(0, std::memory_order_release);
    c.tau128 = (float)tau[0];
    c.tau64 = (float)tau[1];
    c.x0 = (float)x0;
    c.bytes_per_us = (float)bpu;
    c.valid.store(1, std::memory_order_release);
  }
  if (out4) {
    out4[0] = (float)tau[0];
    out4[1] = (float)tau[1];
    out4[2] = (float)x0;
    out4[3] = (float)bpu;
  }
  return ok ? LC_OK : LC_ERR_ARG;
}

int lc_clock_probe(void* out_u64x2, void* stream) {
  if (!out_u64x2) return LC_ERR_ARG;
  return launch_clock_probe(static_cast<unsigned long long*>(out_u64x2), static_cast<hipStream_t>(stream));
}

}  // extern "C"

// every unit with slow-path counters: the MHA units, then the grouped-query ones (the last unit with an offender sets out4[3])
extern "C" int lc_attn_slowpath_stats(unsigned* out4, int reset) {
  for (int gqa = 0; gqa < 2; ++gqa) {
    if (int rc = kAttnW4iUnits[gqa]->slowpath(out4, reset)) return rc;
    for (const AttnW4uUnit* u : kAttnW4uUnits)
      if (u->gqa == (gqa != 0))
        if (int rc = u->slowpath(out4, reset)) return rc;
  }
  return LC_OK;
}
