// tu_attn_varlen_paged_bf16.hip — the bfloat16 ragged-batch kernels over the 16-bit paged cache (attn_varlen_paged_bf16_kernel<D, RT>,
// attn_varlen_chunk_paged_bf16_kernel<D>) and attn_varlen_combine_bf16_kernel<D>, which serves both cache kinds
#define VARLEN_CACHE DecodeCache::PAGED
#define VARLEN_BF16 true
#define VARLEN_OUT VarlenOut::PLAIN
#define VARLEN_COMBINE
#include "tu_attn_varlen_impl.h"
