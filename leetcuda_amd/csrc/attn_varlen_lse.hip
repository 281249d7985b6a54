// attn_varlen_lse.hip — the ragged-batch kernels of attn_varlen.hip / attn_varlen_bf16.hip that also hand back each row's log-sum-exp
// (lc_attn_varlen_paged_lse_f16 / _lse_kv8 / _lse_bf16 / _lse_kv8_bf16): the softmax state a caller needs to merge two
// attention results over disjoint key sets — a shared prefix and the private suffixes (cascade attention), KV shards, a window and a global pass.
// The shared body with LSE = true, which adds ONE store and nothing else: where wave 0 writes a row's O (S = 1), the h = 0 lanes write
//   lse[row] = l > 0 ? (m + log2 l) ln 2 : -inf        row = t H + head, the global row of O
// the NATURAL log of the sum of exp(score) over the row's visible keys, the sink included; score = q.k / sqrt(D) (x k_scale: fp8 pools), v_scale
// does not enter.  With S > 1 the range kernels write part_lse as they always did, and attn_varlen_combine_lse_kernel<D> / _lse_bf16_kernel<D> —
// statement for statement the combine kernels of attn_varlen.hip / attn_varlen_bf16.hip — store lse next to O.  O is the twin's, bit for bit.
// Each kernel takes its twin's arguments with `lse` (device float[T H]) behind them.  Rows nobody owns are written in neither buffer.
#pragma once
#include "attn_varlen_bf16.hip"

namespace lc {

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_lse_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                    const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                    const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                    float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                    int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                    int num_pages, int lps, int max_pages, int window,
                                                                    const float* __restrict__ sinks, const int* __restrict__ cu_q, int T_rows,
                                                                    float* __restrict__ lse) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
  constexpr bool LSE = true;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_lse_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                          const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                          const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                          float* __restrict__ part_o, float* __restrict__ part_lse, int H,
                                                                          int Hkv, int Nq, int Ncap, int causal, int S, float sl2,
                                                                          long total_rows, int num_pages, int lps, int max_pages, int window,
                                                                          const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                          int T_rows, float* __restrict__ lse) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
  constexpr bool LSE = true;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_kv8_lse_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                        const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                        const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                        const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                        float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                        int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                        int num_pages, int lps, int max_pages, int window,
                                                                        const float* __restrict__ sinks, const int* __restrict__ cu_q, int T_rows,
                                                                        float* __restrict__ lse) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
  constexpr bool LSE = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  // (the body takes the pools as byte bases only: page_base)
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kv8_lse_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                              const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                              const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                              const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                              float* __restrict__ part_o, float* __restrict__ part_lse, int H,
                                                                              int Hkv, int Nq, int Ncap, int causal, int S, float sl2,
                                                                              long total_rows, int num_pages, int lps, int max_pages, int window,
                                                                              const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                              int T_rows, float* __restrict__ lse) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = false;
  constexpr bool LSE = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
#include "attn_decode_body.inc"
}

// ---- the bfloat16 forms (BF16 = true: attn_varlen_bf16.hip's four places, and the same one store)

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_lse_bf16_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                         const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                         const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                         float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv,
                                                                         int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
                                                                         int num_pages, int lps, int max_pages, int window,
                                                                         const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                         int T_rows, float* __restrict__ lse) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  constexpr bool LSE = true;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_lse_bf16_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ Kpool,
                                                                               const half_t* __restrict__ Vpool, half_t* __restrict__ O,
                                                                               const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                               float* __restrict__ part_o, float* __restrict__ part_lse, int H,
                                                                               int Hkv, int Nq, int Ncap, int causal, int S, float sl2,
                                                                               long total_rows, int num_pages, int lps, int max_pages, int window,
                                                                               const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                               int T_rows, float* __restrict__ lse) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = false;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  constexpr bool LSE = true;
  const DecodeKv8 kv8{};
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = Kpool;
  const half_t* __restrict__ V = Vpool;
#include "attn_decode_body.inc"
}

template <int D, int RT>
__global__ __launch_bounds__(256) void attn_varlen_paged_kv8_lse_bf16_kernel(const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8,
                                                                             const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
                                                                             const int* __restrict__ kv_len, const int* __restrict__ block_table,
                                                                             const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                                             float* __restrict__ part_o, float* __restrict__ part_lse, int H,
                                                                             int Hkv, int Nq, int Ncap, int causal, int S, float sl2,
                                                                             long total_rows, int num_pages, int lps, int max_pages, int window,
                                                                             const float* __restrict__ sinks, const int* __restrict__ cu_q,
                                                                             int T_rows, float* __restrict__ lse) {
  constexpr bool CHUNK = false;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  constexpr bool LSE = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
#include "attn_decode_body.inc"
}

template <int D>
__global__ __launch_bounds__(256) void attn_varlen_chunk_paged_kv8_lse_bf16_kernel(
    const half_t* __restrict__ Q, const uint8_t* __restrict__ Kpool8, const uint8_t* __restrict__ Vpool8, half_t* __restrict__ O,
    const int* __restrict__ kv_len, const int* __restrict__ block_table, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    float* __restrict__ part_o, float* __restrict__ part_lse, int H, int Hkv, int Nq, int Ncap, int causal, int S, float sl2, long total_rows,
    int num_pages, int lps, int max_pages, int window, const float* __restrict__ sinks, const int* __restrict__ cu_q, int T_rows,
    float* __restrict__ lse) {
  constexpr int RT = 4;
  constexpr bool CHUNK = true;
  constexpr bool LOCAL = true;
  constexpr bool PAGED = true;
  constexpr bool KV8 = true;
  constexpr bool VARLEN = true;
  constexpr bool BF16 = true;
  constexpr bool LSE = true;
  const DecodePaging pg{block_table, num_pages, lps, max_pages};
  const DecodeKv8 kv8{k_scale, v_scale};
  const DecodeLocal lc{window, sinks};
  const DecodeVarlen vl{cu_q, T_rows};
  const DecodeLse ls{lse};
  constexpr bool TREE = false;
  const DecodeTree tr{};
  const half_t* __restrict__ K = reinterpret_cast<const half_t*>(Kpool8);
  const half_t* __restrict__ V = reinterpret_cast<const half_t*>(Vpool8);
#include "attn_decode_body.inc"
}

// attn_varlen_combine_kernel<D> with the row's log-sum-exp: the same merge of the S partials in the same order for the same rows (same O bits),
// and the row's first thread stores lse[row] = (mx + log2 ws) ln 2 — part_lse is in the log2 domain, ws = sum_s exp2(part_lse_s - mx) — or -inf
// for a row whose every range met no key.  A kernel of its own, statement for statement attn_varlen_combine_kernel: that kernel keeps its code
template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_lse_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                      half_t* __restrict__ O, const int* __restrict__ cu_q, int B, int T_rows,
                                                                      int H, int S, float* __restrict__ lse) {
  constexpr int TPR = D / 4;   // threads per row
  const long row = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  const int d = (threadIdx.x % TPR) * 4;
  const int beg = cu_q[0], end = cu_q[B];
  const long total_rows = (long)T_rows * H;
  if (row < (long)(beg < 0 ? 0 : (beg > T_rows ? T_rows : beg)) * H) return;
  if (row >= (long)(end < 0 ? 0 : (end > T_rows ? T_rows : end)) * H) return;
  float mx = DEC_NEG_INF;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, part_lse[(long)s * total_rows + row]);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  float ws = 0.f;
  if (mx != DEC_NEG_INF) {
    for (int s = 0; s < S; ++s) {
      const float wgt = __builtin_amdgcn_exp2f(part_lse[(long)s * total_rows + row] - mx);
      if (wgt > 0.f) {
        acc += *reinterpret_cast<const f32x4_t*>(part_o + ((long)s * total_rows + row) * D + d) * wgt;
        ws += wgt;
      }
    }
  }
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  half4_t y = {(half_t)(acc[0] * inv), (half_t)(acc[1] * inv), (half_t)(acc[2] * inv), (half_t)(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * D + d) = y;
  if (d == 0) lse[row] = mx == DEC_NEG_INF ? DEC_NEG_INF : (mx + log2f(ws)) * 0.6931471805599453f;
}

// ... and attn_varlen_combine_bf16_kernel<D> with the same store
template <int D>
__global__ __launch_bounds__(256) void attn_varlen_combine_lse_bf16_kernel(const float* __restrict__ part_o, const float* __restrict__ part_lse,
                                                                           half_t* __restrict__ O, const int* __restrict__ cu_q, int B,
                                                                           int T_rows, int H, int S, float* __restrict__ lse) {
  constexpr int TPR = D / 4;   // threads per row
  const long row = (long)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  const int d = (threadIdx.x % TPR) * 4;
  const int beg = cu_q[0], end = cu_q[B];
  const long total_rows = (long)T_rows * H;
  if (row < (long)(beg < 0 ? 0 : (beg > T_rows ? T_rows : beg)) * H) return;
  if (row >= (long)(end < 0 ? 0 : (end > T_rows ? T_rows : end)) * H) return;
  float mx = DEC_NEG_INF;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, part_lse[(long)s * total_rows + row]);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  float ws = 0.f;
  if (mx != DEC_NEG_INF) {
    for (int s = 0; s < S; ++s) {
      const float wgt = __builtin_amdgcn_exp2f(part_lse[(long)s * total_rows + row] - mx);
      if (wgt > 0.f) {
        acc += *reinterpret_cast<const f32x4_t*>(part_o + ((long)s * total_rows + row) * D + d) * wgt;
        ws += wgt;
      }
    }
  }
  const float inv = ws > 0.f ? 1.f / ws : 0.f;
  half4_t y = {cvt16<true>(acc[0] * inv), cvt16<true>(acc[1] * inv), cvt16<true>(acc[2] * inv), cvt16<true>(acc[3] * inv)};
  *reinterpret_cast<half4_t*>(O + row * D + d) = y;
  if (d == 0) lse[row] = mx == DEC_NEG_INF ? DEC_NEG_INF : (mx + log2f(ws)) * 0.6931471805599453f;
}

}  // namespace lc
