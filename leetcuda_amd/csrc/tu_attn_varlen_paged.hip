// tu_attn_varlen_paged.hip — the fp16 ragged-batch kernels over the fp16 paged cache (attn_varlen_paged_kernel<D, RT>,
// attn_varlen_chunk_paged_kernel<D>) and attn_varlen_combine_kernel<D>, which serves both cache kinds
#define VARLEN_CACHE DecodeCache::PAGED
#define VARLEN_BF16 false
#define VARLEN_OUT VarlenOut::PLAIN
#define VARLEN_COMBINE
#include "tu_attn_varlen_impl.h"
