// tu_attn_varlen_paged_kv8_lse_bf16.hip — the bfloat16 ragged-batch kernels over the fp8 paged cache that also write each row's log-sum-exp
// (attn_varlen_paged_kv8_lse_bf16_kernel<D, RT>, attn_varlen_chunk_paged_kv8_lse_bf16_kernel<D>).  The combine kernel is
// tu_attn_varlen_paged_lse_bf16.hip's
#define VARLEN_CACHE DecodeCache::PAGED_KV8
#define VARLEN_BF16 true
#define VARLEN_OUT VarlenOut::LSE
#include "tu_attn_varlen_impl.h"
