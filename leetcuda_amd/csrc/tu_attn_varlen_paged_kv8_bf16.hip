// tu_attn_varlen_paged_kv8_bf16.hip — the bfloat16 ragged-batch kernels over the fp8 paged cache (attn_varlen_paged_kv8_bf16_kernel<D, RT>,
// attn_varlen_chunk_paged_kv8_bf16_kernel<D>).  The combine kernel is tu_attn_varlen_paged_bf16.hip's
#define VARLEN_CACHE DecodeCache::PAGED_KV8
#define VARLEN_BF16 true
#define VARLEN_OUT VarlenOut::PLAIN
#include "tu_attn_varlen_impl.h"
