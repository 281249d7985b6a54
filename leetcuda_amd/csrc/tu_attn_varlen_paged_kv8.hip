// tu_attn_varlen_paged_kv8.hip — the fp16 ragged-batch kernels over the fp8 paged cache (attn_varlen_paged_kv8_kernel<D, RT>,
// attn_varlen_chunk_paged_kv8_kernel<D>).  The combine kernel is tu_attn_varlen_paged.hip's
#define VARLEN_CACHE DecodeCache::PAGED_KV8
#define VARLEN_BF16 false
#define VARLEN_OUT VarlenOut::PLAIN
#include "tu_attn_varlen_impl.h"
